"""The lasso's penalty family restated in NumPy (a helper of test_penalty_host / test_gpu_penalty, not a test):

    minimise 1/2*||D*x - s||^2 + g(z)  subject to x - z = 0,
    g(z) = lambda1*sum_i w_i*|z_i| + lambdaG*sum_g omega_g*||z_g||_2 + mu/2*||z||^2 + [z >= 0 when nonnegative]

Without groups lambda1 is the problem's lambda; with groups lambdaG is, and lambda1 is the separate field l1.  The
oracle's admm runs with the lasso x-update of oracle.proxops_ref.getproxops("LASSO", ...) and, as the caller's zming,
prox_{g/rho}(v), v = x + u:

    1. e_i = sign(v_i)*max(|v_i| - tau_i, 0), tau_i = (lambda1/rho)*w_i      (nonnegative: e_i = max(v_i - tau_i, 0))
    2. with groups: e_g *= (||e_g|| > t_g ? 1 - t_g/||e_g|| : 0), t_g = (lambdaG/rho)*omega_g
    3. z = kappa*e, kappa = rho/(rho + mu)

The l1 term, the group term and the orthant's indicator are positively homogeneous: the prox of (a radial norm + such a
term) is shrink o (soft / positive part), and adding mu/2*||.||^2 to a positively homogeneous f/rho scales its prox by
kappa.  test_penalty_host checks the optimality conditions instead of trusting this."""
import numpy as np
import scipy.linalg as sla

import grouplasso_restated as G
from oracle import admm_ref
from oracle.proxops_ref import getproxops

EPS = float(np.finfo(np.float64).eps)
SIZES = [1, 127, 1, 200, 3, 300, 68]  # tests/test_gpu_grouplasso.py: what each size is there for


class Penalty:
    """one member of the family; ``sizes`` None: no groups (l1 is not read then)"""

    def __init__(self, l1weights=None, ridge=0.0, nonnegative=0, sizes=None, groupweights=None, l1=0.0):
        self.w = None if l1weights is None else np.asarray(l1weights, dtype=np.float64)
        self.ridge, self.nonnegative, self.l1 = float(ridge), int(nonnegative), float(l1)
        self.sizes = None if sizes is None else [int(p) for p in sizes]
        self.gw = None if groupweights is None else np.asarray(groupweights, dtype=np.float64)

    def lambda1(self, lam):
        return lam if self.sizes is None else self.l1

    def options(self):
        """the fields as ap.lasso / ap.grouplasso read them from options"""
        o = {}
        if self.w is not None:
            o["l1weights"] = self.w
        if self.ridge:
            o["ridge"] = self.ridge
        if self.nonnegative:
            o["nonnegative"] = 1
        if self.sizes is not None:
            if self.l1:
                o["l1"] = self.l1
            if self.gw is not None:
                o["groupweights"] = self.gw
        return o


def soft(v, tau, nonnegative=0):
    """stage 1 in the arithmetic form of the device's soft(): tau = 0 returns v bit for bit (max(v, 0) when nonnegative)"""
    if nonnegative:
        a = v - tau
        return np.where(a > 0, a, np.zeros_like(a))
    a = np.abs(v) - tau
    p = np.where(a > 0, a, np.zeros_like(a))
    return np.where(v > 0, p, np.where(v < 0, -p, 0 * p))


def prox(v, pen, tau, t, rho, dtype=np.float64):
    """prox_{g/rho}(v) with tau = lambda1/rho and t = lambdaG/rho given as the fp64 numbers the device gets; dtype =
    np.longdouble gives the value fp64 results are measured against"""
    v = np.asarray(v, dtype=dtype)
    w = np.ones(v.size, dtype=dtype) if pen.w is None else pen.w.astype(dtype)
    e = soft(v, dtype(tau) * w, pen.nonnegative)
    if pen.sizes is not None:
        e = G.shrink(e, pen.sizes, t, pen.gw, dtype=dtype)
    return dtype(rho) / (dtype(rho) + dtype(pen.ridge)) * e


def g_of(z, pen, lam):
    """g(z) without the indicator"""
    w = 1.0 if pen.w is None else pen.w
    val = pen.lambda1(lam) * float(np.sum(w * np.abs(z))) + 0.5 * pen.ridge * float(np.sum(z * z))
    if pen.sizes is not None:
        val += lam * G.penalty(z, pen.sizes, pen.gw)
    return val


def objective(D, s, lam, pen, x, z):
    return 0.5 * float(np.sum((D @ x - s) ** 2)) + g_of(z, pen, lam)


def run(D, s, lam, pen, options=None):
    """the serial branch of lasso.m:159-192 and 227-239 with this z-update (as grouplasso_restated.run)"""
    options = dict(options or {})
    rho = float(options.get("rho", 1.0))
    m, n = D.shape
    L = sla.cholesky(D.T @ D + rho * np.eye(n), lower=True) if m >= n else sla.cholesky((D @ D.T) / rho + np.eye(m), lower=True)
    args = dict(D=D, Dts=D.T @ s, L=L, U=L.T, m=m, n=n, parallel=0, rho=rho)
    args["lambda"] = lam
    minx, _, _ = getproxops("LASSO", args)
    zming = lambda x, _z, u, r: prox(x + u, pen, pen.lambda1(lam) / r, lam / r, r)
    options["obj"] = lambda x, z: objective(D, s, lam, pen, x, z)
    options.update(A=1, At=1, m=n, nA=n, nB=n, B=-1, c=0, parallel="none")
    return admm_ref.admm(minx, zming, options)


def bound_ratio(v, got, exact, pen, tau):
    """worst |got_i - exact_i| / ((p_g + 12)*eps*(|v_i| + tau_i)) over the elements, p_g = 1 without groups: the rounding
    of each operation of the chain (tau*w_i, the subtraction, a p_g-term sum of squares, root, division, subtraction, the
    two products and kappa) relative to the sizes that enter it.  Where the bound is 0 the result must be exact."""
    n = len(v)
    p = np.ones(n)
    if pen.sizes is not None:
        p = np.repeat(np.asarray(pen.sizes, dtype=np.float64), pen.sizes)
    taui = tau * (np.ones(n) if pen.w is None else pen.w)
    bound = ((p + 12) * EPS).astype(np.longdouble) * (np.abs(v).astype(np.longdouble) + taui.astype(np.longdouble))
    d = np.abs(np.asarray(got, dtype=np.longdouble) - exact)
    assert np.all(d[bound == 0] == 0)
    nz = bound > 0
    return float(np.max(d[nz] / bound[nz])) if nz.any() else 0.0


# ------------------------------------------------------------------------------------ the fixtures of the GPU tests
KINDS = ("weights", "ridge", "nonnegative", "all", "sparsegroup")
SEEDS = dict(tall=3, wide=4, rows=9)  # 1024 x 700, 512 x 700 (fat), 2000 x 1600


def fixture(synth, kind, rows, cols, seed, sizes=None):
    """lassotest's problem (synth.lasso_problem: unit columns, a 60 %-dense truth of both signs, lambda = 0.1*||D's||_inf)
    with one member of the family.  Weights: uniform in [0.5, 2] with one zero (an unpenalised coefficient).
    sparsegroup: a group-sparse truth with zeros inside the live groups, sqrt(p_g) group weights, lambdaG = a tenth of the
    smallest one that zeroes every group, l1 = half of lasso's lambda, and a ridge term."""
    p = synth.lasso_problem(seed, rows, cols)
    D, s, lam = p["D"], p["s"], p["lam"]
    rng = np.random.default_rng(seed + 500)
    w = rng.uniform(0.5, 2.0, cols)
    w[min(5, cols - 1)] = 0.0
    if kind == "weights":
        pen = Penalty(l1weights=w)
    elif kind == "ridge":
        pen = Penalty(ridge=0.5)
    elif kind == "nonnegative":
        pen = Penalty(nonnegative=1)
    elif kind == "all":
        pen = Penalty(l1weights=w, ridge=0.5, nonnegative=1)
    elif kind == "sparsegroup":
        sizes = list(SIZES if sizes is None else sizes)
        assert sum(sizes) == cols
        off = G.offsets(sizes)
        xt = np.zeros(cols)
        for g in (1, 3, 7):
            if g < len(sizes):
                xg = rng.standard_normal(sizes[g])
                xg[rng.random(sizes[g]) < 0.5] = 0.0
                xt[off[g]:off[g + 1]] = xg
        s = D @ xt + np.sqrt(0.001) * rng.standard_normal(rows)
        gw = np.sqrt(np.asarray(sizes, dtype=np.float64))
        g0 = D.T @ s
        l1 = 0.05 * float(np.max(np.abs(g0)))
        lam = 0.1 * max(float(np.linalg.norm(soft(g0[off[g]:off[g + 1]], l1))) / gw[g] for g in range(len(sizes)))
        pen = Penalty(ridge=0.25, sizes=sizes, groupweights=gw, l1=l1)
    else:
        raise ValueError(kind)
    return dict(D=D, s=s, lam=lam, pen=pen, kind=kind)
