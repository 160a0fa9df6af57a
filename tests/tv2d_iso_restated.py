"""Isotropic 2-D total variation restated in NumPy (a helper of test_tv2d_iso_host / test_gpu_tv2d_iso, not a test):

    minimise 1/2*||x - s||^2 + lambda * sum_k sqrt((Dx)[k]^2 + (Dx)[N+k]^2),   k over the N = H*W pixels,

with D = [Dv; Dh] of oracle.solvers_ref.tv2d_operator (a difference that leaves the image is a zero row of D).  The
oracle's admm runs with the sparse-LU x-update of oracle.solvers_ref.totalvariation2d and, as zming, the block soft
threshold of every pixel's pair of differences -- the pixels of the last image row / column included --

    v = u + D x,   n_k = sqrt(v[k]^2 + v[N+k]^2),   c_k = n_k > t ? 1 - t/n_k : 0,   z[k] = c_k v[k],  z[N+k] = c_k v[N+k]

with t = lambda/rho, written in exactly this form: t = 0 returns v bit for bit and n_k = 0 never divides."""
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import admm_ref
from oracle.solvers_ref import tv2d_operator


def shrink_pair(v, t):
    """the pair shrink of a 2N-vector whose halves are paired"""
    v = np.asarray(v, dtype=np.float64)
    N = v.size // 2
    v0, v1 = v[:N], v[N:]
    n = np.sqrt(v0 * v0 + v1 * v1)
    c = np.zeros(N)
    big = n > t
    c[big] = 1.0 - t / n[big]
    return np.concatenate([c * v0, c * v1])


def penalty(d):
    """sum_k ||(d[k], d[N+k])||_2 of a 2N-vector"""
    N = d.size // 2
    return float(np.sum(np.sqrt(d[:N] * d[:N] + d[N:] * d[N:])))


def objective(img, lam, X):
    """1/2*||X - S||_F^2 + lambda * the isotropic TV of the image X"""
    img, X = np.asarray(img, dtype=np.float64), np.asarray(X, dtype=np.float64)
    H, W = img.shape
    D = tv2d_operator(H, W)
    x = X.reshape(-1, order="F")
    return 0.5 * float(np.sum((x - img.reshape(-1, order="F")) ** 2)) + lam * penalty(D @ x)


def run(S, lam, options=None):
    """oracle.solvers_ref.totalvariation2d with the pair prox and the isotropic objective"""
    options = dict(options or {})
    t0 = time.perf_counter()
    img = np.asarray(S, dtype=np.float64)
    H, W = img.shape
    N = H * W
    s = img.reshape(-1, order="F")
    D = tv2d_operator(H, W)
    Dt = D.T.tocsr()
    rho = float(options.get("rho", 1.0))
    lu = spla.splu((sp.identity(N, format="csc") + rho * (Dt @ D)).tocsc())
    xmin = lambda _x, z, u, r_: lu.solve(s + r_ * (Dt @ (z - u)))
    zmin = lambda x, _z, u, r_: shrink_pair(u + D @ x, lam / r_)
    options.update(A=D, At=Dt, B=-1, nA=N, nB=2 * N, c=0, m=2 * N)
    options["obj"] = lambda x, z: 0.5 * float(np.sum((x - s) ** 2)) + lam * penalty(D @ x)
    results = admm_ref.admm(xmin, zmin, options)
    results["xopt"] = results["xopt"].reshape((H, W), order="F")
    results["solverruntime"] = time.perf_counter() - t0
    return results
