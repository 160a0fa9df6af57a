"""The multi-fit robust regression with a matrix-free x-update restated in NumPy (a helper of test_sparse_reg_host /
test_gpu_sparse_reg, not a test): the oracle's admm() loop with the operators and options lad.m:134-148 /
huberfit.m:166-180 set up (A = D, B = -1, c = s, stopcond 'standard'), whose x-update (D'D)^-1 D'(s + z - u) is
sparse_svm_restated.CgPinv -- conjugate gradients on D'D x = D'(s + z - u), the first solve of a run from 0, every later
one from the previous x -- and whose z-prox and objective are loss_restated's.

Also the problems of the sparse-regression tests: sparse_cases.problem's matrices (row 3 dense, row 5 empty, unit
columns) whose empty column 7 gets one entry, so that rank = n and the oracle's chol(D'D) exists; the seven fits of
reg_multi_cases.FITS in the three modes shared / per-fit S / weighted; per-fit starts z0, u0."""
import numpy as np

import loss_restated as LR
from oracle import admm_ref
from reg_multi_cases import FITS, MODES, loss_of
from sparse_svm_restated import CgPinv

FIELDS = ("xopt", "zopt", "uopt", "pnorm", "perr", "dnorm", "derr", "objevals", "objopt")
HIST = ("pnorm", "perr", "dnorm", "derr", "objevals")

# the largest relative gap between the restatement (cg_tol = 1e-13) and the oracle over SHAPES x MODES x FITS x
# nodualerror 1 | 0 x FIELDS, as test_sparse_reg_host.test_restatement_matches_the_oracle_and_measures_the_parity_gap
# printed it; the device's bound is 10x this (q37's margin: its summation order inside the products)
MEASURED_GAP = 2.6e-9  # 2.585e-09: the epsilon-insensitive fit on 600x120, per-fit S, nodualerror = 0
PARITY_BOUND = 10.0 * MEASURED_GAP
assert PARITY_BOUND <= 1e-6  # never looser than the project's parity definition

SHAPES = ((600, 120, 0.05), (257, 65, 0.03))
SEEDS = {(600, 120, 0.05): 3, (257, 65, 0.03): 3}  # chosen on the CPU: the fits' oracle runs stop at different steps
FILL_ROW = 11  # the row of the one entry that column 7 gets
DUAL_MAXITERS = 400  # of the runs with nodualerror = 0: the dual residual of a LAD fit falls slowly (the oracle's default
                     # lad takes the full 1000 iterations here), and the Huber fits stop on both residuals long before


def run(D, s, loss, options=None, cg_tol=1e-12, cg_maxit=200):
    """one fit: results of the oracle's admm() plus cg_iters_total and cg_capped_updates"""
    D = np.asarray(D, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    m, n = D.shape
    cg = CgPinv(D, cg_tol, cg_maxit)
    o = dict(options or {})
    o.update(A=D, B=-1, c=s, m=m, nA=n, nB=m, obj=lambda x, z: LR.g_of(z, loss))
    res = admm_ref.admm(lambda x, z, u, rho: cg(x, s + z, u, rho),  # y = D'((s + z) - u)
                        lambda x, _z, u, rho: LR.prox(D @ x + u - s, loss, rho), o)
    res["cg_iters_total"], res["cg_capped_updates"] = cg.total, cg.capped
    return res


def oracle_run(D, s, fit, weights, options):
    """the reference side of the parity tests: oracle.solvers_ref.lad / huberfit where the oracle has the loss (the
    plain members without weights), else the oracle's loop with the restated prox (loss_restated.run)"""
    from oracle import solvers_ref as S
    loss = loss_of(fit, weights)
    plain = weights is None and (loss.a, loss.b, loss.eps, loss.delta) == (1.0, 1.0, 0.0, 1.0)
    if plain:
        return (S.lad if loss.kind == "lad" else S.huberfit)(D, s, dict(options))
    return LR.run(loss.kind, D, s, loss, dict(options))


def relgap(got, ref, steps=None):
    """the largest relative gap over FIELDS by sparse_svm_restated.relgap's measure: scalar histories per entry against
    max(|ref|, 1e-12 + 1e-3 max|ref|), everything else against max|ref|.  A history that is NaN in the reference
    (dnorm / derr under nodualerror = 1) is not a field of that run."""
    worst = 0.0
    for key in FIELDS:
        if key not in ref or (key in ("dnorm", "derr") and np.isnan(np.asarray(ref[key], dtype=np.float64)).all()):
            continue
        a, b = np.atleast_1d(np.asarray(got[key], dtype=np.float64)), np.atleast_1d(np.asarray(ref[key], dtype=np.float64))
        if steps is not None and key in HIST:
            a, b = a[:steps], b[:steps]
        assert a.shape == b.shape, (key, a.shape, b.shape)
        assert not np.isnan(a).any() and not np.isnan(b).any(), key
        if b.ndim == 1 and not key.endswith("opt"):
            err = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-12 + 1e-3 * np.max(np.abs(b)))))
        else:
            err = float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))
        worst = max(worst, err)
    return worst


# ---- the problems
_CACHE = {}
_REFS = {}


def matrix(ap, rows, cols, density, full_rank=True):
    """sparse_cases.problem's matrix as a dense array; full_rank: column 7 gets the entry (FILL_ROW, 7) = 1"""
    from sparse_cases import problem as lasso_problem
    A = lasso_problem(ap, rows, cols, density, seed=SEEDS.get((rows, cols, density), 3))["A"].copy()
    if full_rank and cols > 7:
        assert not A[:, 7].any()
        A[FILL_ROW, 7] = 1.0
    return np.asfortranarray(A)


def case(ap, shape, mode, A=None):
    """dict(D csc_matrix, A dense, S m x 1 | m x 7, w, z0, u0 m x 7) of one (shape, mode); A: another matrix of the
    test's own (the rank-deficient ones) in place of matrix(ap, *shape)"""
    import scipy.sparse as sp
    key = (shape, mode)
    if A is not None or key not in _CACHE:
        own = A is not None
        if not own:
            A = matrix(ap, *shape)
            assert np.linalg.matrix_rank(A) == A.shape[1]  # the oracle's lad calls a Cholesky and needs it
        m, n = A.shape
        K = len(FITS)
        rng = np.random.default_rng(SEEDS.get(tuple(shape), 3) + 1300)
        xtrue = rng.standard_normal(n)
        s = A @ xtrue + 0.3 * (1.0 + 0.5 * np.abs(rng.standard_normal(m))) * rng.standard_normal(m)
        if mode == "perfit":
            S = np.asfortranarray(np.column_stack([(1.0 + 0.15 * k) * s + 0.2 * k + 0.3 * rng.standard_normal(m)
                                                   for k in range(K)]))
        else:
            S = np.asfortranarray(s.reshape(-1, 1))
        w = None
        if mode == "weighted":
            w = rng.uniform(0.5, 2.0, m)
            w[::7] = 0.0  # observations that do not count
        z0, u0 = (np.asfortranarray(0.5 * rng.standard_normal((m, K))) for _ in range(2))
        c = dict(D=sp.csc_matrix(A), A=A, S=S, w=w, z0=z0, u0=u0)
        if own:
            return c
        _CACHE[key] = c
    return _CACHE[key]


TALL = (8200, 40, 0.02)  # more than 32 * 256 rows: a workgroup of the element pass takes two row blocks
TALL_FITS = (0, 1, 4)
TALL_MAXITERS = 40


def tall_case(ap):
    if "tall" not in _CACHE:
        A = matrix(ap, *TALL)
        assert np.linalg.matrix_rank(A) == A.shape[1]
        _CACHE["tall"] = case(ap, TALL, "shared", A=A)
    return _CACHE["tall"]


def tall_oracle(ap, k):
    if ("tall", k) not in _REFS:
        c = tall_case(ap)
        _REFS[("tall", k)] = oracle_run(c["A"], response(c, k), FITS[k], None, fit_options(c, k, 1, maxiters=TALL_MAXITERS))
    return _REFS[("tall", k)]


def loop_options(nodualerror):
    return dict(objevals=1, nodualerror=nodualerror, **({} if nodualerror else dict(maxiters=DUAL_MAXITERS)))


def fit_options(c, k, nodualerror, **more):
    return dict(loop_options(nodualerror), z0=c["z0"][:, k], u0=c["u0"][:, k], **more)


def response(c, k):
    return np.ascontiguousarray(c["S"][:, k if c["S"].shape[1] > 1 else 0])


def oracle_fit(ap, shape, mode, k, nodualerror):
    """the oracle's run of fit k of (shape, mode), computed once"""
    key = (shape, mode, k, nodualerror)
    if key not in _REFS:
        c = case(ap, shape, mode)
        _REFS[key] = oracle_run(c["A"], response(c, k), FITS[k], c["w"], fit_options(c, k, nodualerror))
    return _REFS[key]


def restated_fit(c, k, nodualerror, **more):
    return run(c["A"], response(c, k), loss_of(FITS[k], c["w"]), fit_options(c, k, nodualerror, **more), cg_tol=1e-13)
