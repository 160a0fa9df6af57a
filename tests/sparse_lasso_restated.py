"""The multi-fit lasso with a matrix-free x-update restated in NumPy (a helper of test_sparse_lasso_host /
test_gpu_sparse_lasso, not a test): the oracle's admm() loop with the operators and options lasso.m:227-239
sets up (A = 1, B = -1, c = 0, sizes n, stopcond 'standard'), whose x-update (D'D + rho*I)^-1 (D's + rho*(z - u))
(lasso.m:28-30) is conjugate gradients on the shifted normal equations -- the first solve of a run from 0, every later one
from the previous x; a solve ends on ||r|| <= cg_tol*||y||, on cg_maxit, on a zero right-hand side (x = 0) or on p.q = 0 --
and whose z-prox and objective are penalty_restated's (q32's family without groups).

Also the problems of the sparse-lasso tests: sparse_cases.problem's matrices (row 3 dense, row 5 and column 7 empty, unit
columns; rho > 0 makes the oracle's Cholesky exist whatever the rank) and a grid of seven fits per problem."""
import numpy as np

import penalty_restated as PR
from oracle import admm_ref
from sparse_reg_restated import relgap  # noqa: F401 (the measure of q37 / q38, over the same field names)

# the largest relative gap between the restatement (cg_tol = 1e-13) and the oracle over SHAPES x MODES x the seven fits x
# nodualerror 0 | 1 x every field and history entry, as
# test_sparse_lasso_host.test_restatement_matches_the_oracle_and_measures_the_parity_gap printed it; the device's bound is
# 10x this (q37's margin: its summation order inside the products)
MEASURED_GAP = 5.9e-10  # 5.803e-10: the 0.01*lambda_max fit on 80x200 (fat), per-fit S, nodualerror = 0, 327 iterations
PARITY_BOUND = 10.0 * MEASURED_GAP
assert PARITY_BOUND <= 1e-6  # never looser than the project's parity definition

SHAPES = ((600, 120, 0.05), (257, 65, 0.03), (80, 200, 0.10))  # the last one fat: the oracle's other Cholesky branch
SEEDS = {(600, 120, 0.05): 1, (257, 65, 0.03): 1, (80, 200, 0.10): 1}  # chosen on the CPU: the fits stop at >= 5 distinct steps
MODES = ("shared", "perfit")
# lambda_k as a fraction of the fit's own lambda_max = ||D's_k||_inf: lambda = 0, four inside the path, one above
# lambda_max (z = 0 exactly), and an elastic-net fit under the shared l1 weights with the sign constraint
FRACTIONS = (0.0, 0.01, 0.05, 0.2, 0.5, 1.25, 0.1)
RIDGE = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5)
NONNEG = (0, 0, 0, 0, 0, 0, 1)
K = len(FRACTIONS)
PLAIN = (0, 1, 2, 3, 4, 5)  # the fits the oracle's own lasso runs (no weights)
FAMILY = 6                  # the fit that runs under the weights


class CgShift:
    """x-update closure with the solver's state: x of the previous solve, inner iterations, capped solves"""

    def __init__(self, D, Dts, cg_tol=1e-12, cg_maxit=200):
        self.D, self.Dts, self.tol, self.maxit = D, Dts, float(cg_tol), int(cg_maxit)
        self.x, self.total, self.capped = None, 0, 0

    def __call__(self, _x, z, u, rho):
        D = self.D
        y = rho * (z - u) + self.Dts
        if self.x is None:
            x, r = np.zeros(D.shape[1]), y.copy()
        else:
            x = self.x.copy()
            r = y - (D.T @ (D @ x) + rho * x)
        yy, rs = float(y @ y), float(r @ r)
        if yy == 0.0:
            self.x = np.zeros(D.shape[1])
            return self.x.copy()
        ynorm = np.sqrt(yy)
        p = r.copy()
        it, converged = 0, np.sqrt(rs) <= self.tol * ynorm
        while not converged and it < self.maxit:
            q = D.T @ (D @ p) + rho * p
            pq = float(p @ q)
            it += 1
            self.total += 1
            if pq == 0.0:
                break
            alpha = rs / pq
            x = x + alpha * p
            r = r - alpha * q
            rsn = float(r @ r)
            p = r + (rsn / rs) * p
            rs = rsn
            converged = np.sqrt(rs) <= self.tol * ynorm
        if not converged:
            self.capped += 1
        self.x = x
        return x.copy()


def run(D, s, lam, pen, options=None, cg_tol=1e-12, cg_maxit=200):
    """one fit: results of the oracle's admm() plus cg_iters_total and cg_capped_updates"""
    D = np.asarray(D, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    n = D.shape[1]
    cg = CgShift(D, D.T @ s, cg_tol, cg_maxit)
    o = dict(options or {})
    o["obj"] = lambda x, z: PR.objective(D, s, lam, pen, x, z)
    o.update(A=1, At=1, m=n, nA=n, nB=n, B=-1, c=0, parallel="none")
    res = admm_ref.admm(cg, lambda x, _z, u, r: PR.prox(x + u, pen, lam / r, 0.0, r), o)
    res["cg_iters_total"], res["cg_capped_updates"] = cg.total, cg.capped
    return res


def oracle_run(D, s, lam, pen, options):
    """the reference side of the parity tests: oracle.solvers_ref.lasso for a plain fit, else the oracle's loop with the
    restated prox (penalty_restated.run)"""
    from oracle import solvers_ref as S
    if pen.w is None and not pen.ridge and not pen.nonnegative:
        return S.lasso(D, s, lam, dict(options))
    return PR.run(D, s, lam, pen, dict(options))


# ---- the problems
_CACHE = {}
_REFS = {}


def matrix(ap, rows, cols, density):
    from sparse_cases import problem as lasso_problem
    return np.asfortranarray(lasso_problem(ap, rows, cols, density, seed=SEEDS.get((rows, cols, density), 3))["A"])


def case(ap, shape, mode, A=None):
    """dict(D csc_matrix, A dense, S m x 1 | m x K, w, lams, z0, u0 n x K) of one (shape, mode); A: another matrix of the
    test's own in place of matrix(ap, *shape)"""
    import scipy.sparse as sp
    key = (tuple(shape), mode)
    if A is not None or key not in _CACHE:
        own = A is not None
        if not own:
            A = matrix(ap, *shape)
        m, n = A.shape
        rng = np.random.default_rng(SEEDS.get(tuple(shape), 3) + 2600)
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
        # lambda = 0 makes z = x + u exactly, so u and x - z are what rounding leaves of u0: from a nonzero start they are
        # noise of size eps on which no relative measure means anything; from the zero start they are exactly 0.0 in the
        # oracle, in the restatement and on the device, and every entry of every field stays in the comparison
        z0[:, 0] = 0.0
        u0[:, 0] = 0.0
        c = dict(D=sp.csc_matrix(A), A=A, S=S, w=w, lams=lams, lmax=lmax, z0=z0, u0=u0)
        if own:
            return c
        _CACHE[key] = c
    return _CACHE[key]


def penalty_of(c, k, weighted):
    return PR.Penalty(l1weights=c["w"] if weighted else None, ridge=RIDGE[k], nonnegative=NONNEG[k])


def loop_options(nodualerror, **more):
    return dict(objevals=1, nodualerror=nodualerror, **more)


def fit_options(c, k, nodualerror, **more):
    return dict(loop_options(nodualerror), z0=c["z0"][:, k], u0=c["u0"][:, k], **more)


def response(c, k):
    return np.ascontiguousarray(c["S"][:, k if c["S"].shape[1] > 1 else 0])


def weighted_fit(k):
    """fit k runs under the shared weights in the parity tests (the object carries them for all fits of a run)"""
    return k == FAMILY


def oracle_fit(ap, shape, mode, k, nodualerror, **more):
    """the oracle's run of fit k of (shape, mode), computed once"""
    key = (tuple(shape), mode, k, nodualerror, tuple(sorted(more.items())))
    if key not in _REFS:
        c = case(ap, shape, mode)
        _REFS[key] = oracle_run(c["A"], response(c, k), float(c["lams"][k]), penalty_of(c, k, weighted_fit(k)),
                                fit_options(c, k, nodualerror, **more))
    return _REFS[key]


def restated_fit(c, k, nodualerror, weighted=None, **more):
    weighted = weighted_fit(k) if weighted is None else weighted
    return run(c["A"], response(c, k), float(c["lams"][k]), penalty_of(c, k, weighted),
               fit_options(c, k, nodualerror, **more), cg_tol=1e-13)


WIDE = (60, 8300, 0.02)   # more than 32 * 256 coefficients: a workgroup of the element pass takes two row blocks
WIDE_FITS = (1, 3, 5)
WIDE_MAXITERS = 25
TALL = (8200, 40, 0.02)   # more than 32 * 256 rows: a workgroup of the fit kernel takes two row blocks
TALL_FITS = (0, 2, 4)
TALL_MAXITERS = 40


def big_case(ap, shape):
    key = ("big", tuple(shape))
    if key not in _CACHE:
        _CACHE[key] = case(ap, shape, "shared", A=matrix(ap, *shape))
    return _CACHE[key]


def big_oracle(ap, shape, k, maxiters):
    key = ("big", tuple(shape), k)
    if key not in _REFS:
        c = big_case(ap, shape)
        _REFS[key] = oracle_run(c["A"], response(c, k), float(c["lams"][k]), penalty_of(c, k, False),
                                fit_options(c, k, 0, maxiters=maxiters))
    return _REFS[key]
