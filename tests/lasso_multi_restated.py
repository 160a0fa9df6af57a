"""The multi-fit lasso on a dense design matrix restated in NumPy (a helper of test_lasso_multi_host /
test_gpu_lasso_multi, not a test): the oracle's admm() loop with the operators and options lasso.m:227-239
sets up (A = 1, B = -1, c = 0, sizes n, stopcond 'standard'), whose x-update is x = Minv*(D's + rho*(z - u)) with the
EXPLICIT inverse Minv of D'D + rho*I from its Cholesky factor -- the form the device applies -- and whose z-prox and
objective are penalty_restated's (q32's family without groups).  The oracle's own lasso solves with the factor instead.

Also the problems of the dense multi-lasso tests: tall Gaussian matrices with unit columns (synth.lasso_problem's recipe)
and sparse_lasso_restated's grid of seven fits per problem."""
import numpy as np
import scipy.linalg as sla

import penalty_restated as PR
from oracle import admm_ref
from sparse_lasso_restated import (FAMILY, FRACTIONS, K, MODES, NONNEG, PLAIN, RIDGE, fit_options, loop_options,  # noqa: F401
                                   oracle_run, penalty_of, response, weighted_fit)
from sparse_reg_restated import relgap  # noqa: F401 (the measure of q37 - q39, over the same field names)

# the largest relative gap between the restatement and the oracle over SHAPES x MODES x the seven fits x nodualerror
# 0 | 1 x every field and history entry, as test_lasso_multi_host.test_restatement_matches_the_oracle_and_measures_the_
# parity_gap printed it; the device's bound is 10x this (q37's margin: its summation order inside the tiled product)
MEASURED_GAP = 8.2e-12  # 8.193e-12: the 1.25*lambda_max fit on 600x257, per-fit S, both stop rules, 30 iterations
PARITY_BOUND = 10.0 * MEASURED_GAP
assert PARITY_BOUND <= 1e-6  # never looser than the project's parity definition

RHO = 1.0
# two tile rows with n no multiple of 128; three tile rows with one live row in the last; one tile
SHAPES = ((300, 130), (600, 257), (200, 64))
SEEDS = {(300, 130): 2, (600, 257): 1, (200, 64): 1}  # chosen on the CPU: the fits stop at >= 5 distinct steps


class InverseSolve:
    """x-update closure: the explicit inverse of D'D + rho*I, built once from its Cholesky factor"""

    def __init__(self, D, Dts, rho):
        n = D.shape[1]
        self.Dts, self.rho = Dts, float(rho)
        self.Minv = sla.cho_solve(sla.cho_factor(D.T @ D + rho * np.eye(n), lower=True), np.eye(n))
        self.Minv = 0.5 * (self.Minv + self.Minv.T)

    def __call__(self, _x, z, u, rho):
        assert rho == self.rho
        return self.Minv @ (rho * (z - u) + self.Dts)


def run(D, s, lam, pen, options=None, rho=RHO):
    """one fit: results of the oracle's admm()"""
    D = np.asarray(D, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    n = D.shape[1]
    o = dict(options or {})
    o["obj"] = lambda x, z: PR.objective(D, s, lam, pen, x, z)
    o.update(A=1, At=1, m=n, nA=n, nB=n, B=-1, c=0, parallel="none", rho=rho)
    return admm_ref.admm(InverseSolve(D, D.T @ s, rho), lambda x, _z, u, r: PR.prox(x + u, pen, lam / r, 0.0, r), o)


# ---- the problems
_CACHE = {}
_REFS = {}


def matrix(ap, rows, cols, seed=None):
    seed = SEEDS.get((rows, cols), 3) if seed is None else seed
    return np.asfortranarray(ap.synth.lasso_problem(seed, rows, cols)["D"])


def case(ap, shape, mode, seed=None):
    """dict(A dense, S m x 1 | m x K, w, lams, lmax, z0, u0 n x K) of one (shape, mode), sparse_lasso_restated.case's
    recipe on a dense matrix; seed: another seed than the recorded one (not cached)"""
    key = (tuple(shape), mode)
    if seed is not None or key not in _CACHE:
        sd = SEEDS.get(tuple(shape), 3) if seed is None else seed
        A = matrix(ap, *shape, seed=sd)
        m, n = A.shape
        rng = np.random.default_rng(sd + 2600)
        xtrue = np.where(rng.random(n) < 0.3, rng.standard_normal(n), 0.0)
        s = A @ xtrue + 0.05 * rng.standard_normal(m)
        if mode == "perfit":
            S = np.asfortranarray(np.column_stack([(1.0 + 0.15 * k) * s + 0.1 * rng.standard_normal(m) for k in range(K)]))
        else:
            S = np.asfortranarray(s.reshape(-1, 1))
        w = rng.uniform(0.5, 2.0, n)
        w[min(5, n - 1)] = 0.0  # an unpenalised coefficient
        lmax = np.array([float(np.max(np.abs(A.T @ S[:, k if S.shape[1] > 1 else 0]))) for k in range(K)])
        lams = np.asarray(FRACTIONS) * lmax
        z0, u0 = (np.asfortranarray(0.1 * rng.standard_normal((n, K))) for _ in range(2))
        z0[:, 0] = 0.0  # lambda = 0 from the zero start: u and x - z stay exactly 0.0 (sparse_lasso_restated.case)
        u0[:, 0] = 0.0
        c = dict(A=A, S=S, w=w, lams=lams, lmax=lmax, z0=z0, u0=u0)
        if seed is not None:
            return c
        _CACHE[key] = c
    return _CACHE[key]


def oracle_fit(ap, shape, mode, k, nodualerror, **more):
    """the oracle's run of fit k of (shape, mode), computed once"""
    key = (tuple(shape), mode, k, nodualerror, tuple(sorted(more.items())))
    if key not in _REFS:
        c = case(ap, shape, mode)
        _REFS[key] = oracle_run(c["A"], response(c, k), float(c["lams"][k]), penalty_of(c, k, weighted_fit(k)),
                                fit_options(c, k, nodualerror, rho=RHO, **more))
    return _REFS[key]


def restated_fit(c, k, nodualerror, weighted=None, **more):
    weighted = weighted_fit(k) if weighted is None else weighted
    return run(c["A"], response(c, k), float(c["lams"][k]), penalty_of(c, k, weighted),
               fit_options(c, k, nodualerror, **more))
