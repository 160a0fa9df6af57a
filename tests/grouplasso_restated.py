"""Group lasso restated in NumPy (a helper of test_grouplasso_host / test_gpu_grouplasso, not a test):
minimise 1/2*||D*x - s||^2 + lambda*sum_g w_g*||z_g||_2 subject to x - z = 0 over contiguous groups of sizes p_1..p_G.

The oracle's admm runs with the lasso x-update of oracle.proxops_ref.getproxops("LASSO", ...) and, as the caller's zming,
the block soft threshold (Boyd et al., Distributed Optimization and Statistical Learning via ADMM, 6.4.2)

    z_g = v_g * (||v_g|| > t_g ? 1 - t_g/||v_g|| : 0),   v = x + u,   t_g = lambda*w_g/rho

written in exactly this form: t = 0 returns v bit for bit and ||v_g|| = 0 never divides.  The objective is lasso.m:227
with the group term in place of the l1 norm."""
import numpy as np
import scipy.linalg as sla

from oracle import admm_ref
from oracle.proxops_ref import getproxops

EPS = float(np.finfo(np.float64).eps)


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])


def weights_of(sizes, weights=None):
    return np.ones(len(sizes)) if weights is None else np.asarray(weights, dtype=np.float64)


def shrink(v, sizes, t, weights=None, dtype=np.float64):
    """the block soft threshold with thresholds t*w_g; dtype = np.longdouble gives the value fp64 results are measured
    against (the norm then comes from long-double squares summed in long double)"""
    v = np.asarray(v, dtype=dtype)
    w = weights_of(sizes, weights)
    out = np.empty_like(v)
    off = offsets(sizes)
    for g in range(len(sizes)):
        vg = v[off[g]:off[g + 1]]
        nrm = np.sqrt(np.sum(vg * vg))
        tg = dtype(t) * dtype(w[g])
        out[off[g]:off[g + 1]] = vg * ((dtype(1) - tg / nrm) if nrm > tg else dtype(0))
    return out


def penalty(z, sizes, weights=None):
    w = weights_of(sizes, weights)
    off = offsets(sizes)
    return float(sum(w[g] * np.linalg.norm(z[off[g]:off[g + 1]]) for g in range(len(sizes))))


def objective(D, s, lam, sizes, weights, x, z):
    """lasso.m:227 with the group penalty: 1/2*sum((D*x - s).^2) + lambda*sum_g w_g*norm(z_g)"""
    return 0.5 * float(np.sum((D @ x - s) ** 2)) + lam * penalty(z, sizes, weights)


def run(D, s, lam, sizes, options=None, weights=None):
    """the serial branch of lasso.m:159-192 and 227-239 with the group z-update"""
    options = dict(options or {})
    rho = float(options.get("rho", 1.0))
    m, n = D.shape
    assert int(np.sum(sizes)) == n
    L = sla.cholesky(D.T @ D + rho * np.eye(n), lower=True) if m >= n else sla.cholesky((D @ D.T) / rho + np.eye(m), lower=True)
    args = dict(D=D, Dts=D.T @ s, L=L, U=L.T, m=m, n=n, parallel=0, rho=rho)
    args["lambda"] = lam
    minx, _, _ = getproxops("LASSO", args)
    zming = lambda x, _z, u, r: shrink(x + u, sizes, lam / r, weights)
    options["obj"] = lambda x, z: objective(D, s, lam, sizes, weights, x, z)
    options.update(A=1, At=1, m=n, nA=n, nB=n, B=-1, c=0, parallel="none")
    return admm_ref.admm(minx, zming, options)
