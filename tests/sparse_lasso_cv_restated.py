"""The sparse multi-lasso under observation weights and held-out folds restated in NumPy (a helper of
test_sparse_lasso_cv_host / test_gpu_sparse_lasso_cv, not a test).  Fit k minimises

    1/2*sum_i omega_ik*(d_i'x - s_i)^2 + lambda_k*||x||_1,    omega_ik = obsw_i * [fold_i != held_k]

which is exactly the plain lasso on (diag(sqrt(omega_k))*A with the zero-weight rows dropped, sqrt(omega_k)*s):
sparse_lasso_restated.oracle_run on that pair is the oracle.  The restatement is sparse_lasso_restated's loop with the
weighted CG -- D'(omega o (D p)) + rho*p and the right-hand side D'(omega o s) + rho*(z - u) -- as the device runs it.

Also the problems of the tests: sparse_lasso_restated's matrices with three folds, thirteen fits in two chunks (folds
0, 1, 2 at four fractions of the fold's own lambda_max and one fit that holds nothing out), with and without
observation weights in [0.5, 2] that include two exact zeros."""
import numpy as np

import penalty_restated as PR
import sparse_lasso_restated as R
from oracle import admm_ref
from sparse_reg_restated import relgap  # noqa: F401

# the largest relative gap between the restatement (cg_tol = 1e-13) and the oracle over every problem below (SHAPES x
# weights off | on x the thirteen fits x nodualerror 0 | 1, the tall and wide problems, the emptied column and the
# cross-validation's twenty fits) and every field, as
# test_sparse_lasso_cv_host.test_restatement_matches_the_oracle_and_measures_the_parity_gap printed it; the device's
# bound is 10x this (q37's margin: its summation order inside the products)
MEASURED_GAP = 2.8e-9  # 2.789e-9: fit 8 (fold 2 held out at 0.01*lambda_max) on 257x65 under weights, nodualerror = 0, 138 iterations
PARITY_BOUND = 10.0 * MEASURED_GAP
assert PARITY_BOUND <= 1e-6  # never looser than the project's parity definition

SHAPES = ((257, 65, 0.03), (80, 200, 0.10))  # the second one fat: the oracle's other Cholesky branch
NFOLDS = 3
FRACTIONS = (0.01, 0.05, 0.2, 1.25)  # of the fold fit's own lambda_max = ||D'(omega_k o s)||_inf; 1.25: z = 0 exactly
FULL_FRACTION = 0.1                  # the fit that holds nothing out
HELD = tuple(f for f in range(NFOLDS) for _ in FRACTIONS) + (-1,)
K = len(HELD)  # 13: two chunks
ZERO_FITS = tuple(k for k in range(K - 1) if FRACTIONS[k % len(FRACTIONS)] > 1.0)
SEEDS = {(257, 65, 0.03): 1, (80, 200, 0.10): 1}  # chosen on the CPU: the oracle's fits stop at >= 5 distinct steps


class CgShiftWeighted(R.CgShift):
    """sparse_lasso_restated.CgShift on (D' Omega D + rho*I) x = D'(omega o s) + rho*(z - u)"""

    def __init__(self, D, omega, s, cg_tol=1e-12, cg_maxit=200):
        super().__init__(D, D.T @ (omega * s), cg_tol, cg_maxit)
        self.omega = omega

    def __call__(self, _x, z, u, rho):
        D, om = self.D, self.omega
        y = rho * (z - u) + self.Dts
        if self.x is None:
            x, r = np.zeros(D.shape[1]), y.copy()
        else:
            x = self.x.copy()
            r = y - (D.T @ (om * (D @ x)) + rho * x)
        yy, rs = float(y @ y), float(r @ r)
        if yy == 0.0:
            self.x = np.zeros(D.shape[1])
            return self.x.copy()
        ynorm = np.sqrt(yy)
        p = r.copy()
        it, converged = 0, np.sqrt(rs) <= self.tol * ynorm
        while not converged and it < self.maxit:
            q = D.T @ (om * (D @ p)) + rho * p
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


def scaled_pair(A, s, omega):
    """(diag(sqrt(omega)) A, sqrt(omega) s) with the zero-weight rows dropped"""
    rows = omega > 0
    q = np.sqrt(omega[rows])
    return np.asfortranarray(q[:, None] * A[rows]), q * s[rows]


def restated_run(A, s, omega, lam, options=None, cg_tol=1e-13, cg_maxit=200):
    """one fit of the weighted loop: the oracle's admm() results plus cg_iters_total and cg_capped_updates"""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[1]
    pen = PR.Penalty()
    q = np.sqrt(omega)
    As, ss = q[:, None] * A, q * s
    cg = CgShiftWeighted(A, omega, s, cg_tol, cg_maxit)
    o = dict(options or {})
    o["obj"] = lambda x, z: PR.objective(As, ss, lam, pen, x, z)
    o.update(A=1, At=1, m=n, nA=n, nB=n, B=-1, c=0, parallel="none")
    res = admm_ref.admm(cg, lambda x, _z, u, r: PR.prox(x + u, pen, lam / r, 0.0, r), o)
    res["cg_iters_total"], res["cg_capped_updates"] = cg.total, cg.capped
    return res


def oracle_run(A, s, omega, lam, options):
    """the reference: the oracle's own lasso on the scaled row subset"""
    As, ss = scaled_pair(np.asarray(A, dtype=np.float64), s, omega)
    return R.oracle_run(As, ss, lam, PR.Penalty(), options)


def heldout_sums(A, s, obsw, fold, held, z):
    """(sse, weight) of one fit in NumPy: the weighted squared error of z on the rows of fold `held`, and their weight"""
    w = np.ones(A.shape[0]) if obsw is None else obsw
    out = fold == held
    r = A[out] @ z - s[out]
    return float(np.sum(w[out] * r * r)), float(np.sum(w[out]))


# ---- the problems
_CACHE = {}
_REFS = {}


def omega_of(c, k, weighted):
    w = c["obsw"] if weighted else np.ones(c["A"].shape[0])
    return w * (c["fold"] != c["held"][k])


def make_case(A, seed, held, fractions, nfolds=NFOLDS, fold=None):
    """dict(D, A, s, fold, obsw, held, lams[weighted], z0, u0) over the matrix A: `held` and `fractions` per fit"""
    import scipy.sparse as sp
    m, n = A.shape
    rng = np.random.default_rng(seed + 4600)
    xtrue = np.where(rng.random(n) < 0.3, rng.standard_normal(n), 0.0)
    s = A @ xtrue + 0.05 * rng.standard_normal(m)
    if fold is None:
        fold = rng.permutation(m) % nfolds
    obsw = rng.uniform(0.5, 2.0, m)
    obsw[[min(2, m - 1), m // 2]] = 0.0  # two observations of exactly zero weight
    k = len(held)
    c = dict(D=sp.csc_matrix(A), A=A, s=s, fold=np.asarray(fold, dtype=np.int64), obsw=obsw,
             held=np.asarray(held, dtype=np.int64), nfolds=nfolds)
    c["lams"] = {}
    for weighted in (False, True):
        lmax = np.array([float(np.max(np.abs(A.T @ (omega_of(c, j, weighted) * s)))) for j in range(k)])
        c["lams"][weighted] = np.asarray(fractions) * lmax
    c["z0"], c["u0"] = (np.asfortranarray(0.1 * rng.standard_normal((n, k))) for _ in range(2))
    return c


def case(ap, shape):
    key = tuple(shape)
    if key not in _CACHE:
        A = R.matrix(ap, *shape)
        _CACHE[key] = make_case(A, SEEDS.get(key, 3), HELD, FRACTIONS * NFOLDS + (FULL_FRACTION,))
    return _CACHE[key]


def fit_options(c, k, nodualerror, **more):
    return dict(R.loop_options(nodualerror), z0=c["z0"][:, k], u0=c["u0"][:, k], **more)


def oracle_fit(c, tag, k, weighted, nodualerror, **more):
    """the oracle's run of fit k of the case `tag`, computed once"""
    key = (tag, k, weighted, nodualerror, tuple(sorted(more.items())))
    if key not in _REFS:
        _REFS[key] = oracle_run(c["A"], c["s"], omega_of(c, k, weighted), float(c["lams"][weighted][k]),
                                fit_options(c, k, nodualerror, **more))
    return _REFS[key]


def restated_fit(c, k, weighted, nodualerror, **more):
    return restated_run(c["A"], c["s"], omega_of(c, k, weighted), float(c["lams"][weighted][k]),
                        fit_options(c, k, nodualerror, **more))


# several row blocks: the weighted fit kernel and the epilogue past 32 * 256 rows; the per-fit D's past 32 * 256 columns
TALL, TALL_MAXITERS = R.TALL, R.TALL_MAXITERS
TALL_HELD, TALL_FRACTIONS = (0, 1, 2, -1), (0.05, 0.2, 0.01, 0.1)
WIDE, WIDE_MAXITERS = R.WIDE, R.WIDE_MAXITERS
WIDE_HELD, WIDE_FRACTIONS = (0, 2, -1), (0.05, 0.2, 0.1)


def big_case(ap, shape):
    key = ("big", tuple(shape))
    if key not in _CACHE:
        held, frac = (TALL_HELD, TALL_FRACTIONS) if tuple(shape) == TALL else (WIDE_HELD, WIDE_FRACTIONS)
        _CACHE[key] = make_case(R.matrix(ap, *shape), 3, held, frac)
    return _CACHE[key]


EMPTIED_COLUMN = 11


def emptied_case(ap):
    """(257, 65): fold 1 is every row where column EMPTIED_COLUMN of D is nonzero, so the fits that hold fold 1 out see
    an empty column (rho > 0 keeps the system definite)"""
    key = "emptied"
    if key not in _CACHE:
        A = R.matrix(ap, 257, 65, 0.03)
        rng = np.random.default_rng(77)
        fold = np.where(A[:, EMPTIED_COLUMN] != 0.0, 1, rng.choice([0, 2], size=257))
        _CACHE[key] = make_case(A, 5, (1, 1, 0), (0.05, 0.2, 0.05), fold=fold)
    return _CACHE[key]


# ---- the cross-validation of test 7: (600, 120, 0.05), F = 3, L = 5
CV_SHAPE, CV_FOLDS, CV_NLAMBDA = (600, 120, 0.05), 3, 5
# |d cvm| / cvm <= CV_CONDITION * (the relative gap of zopt): with r = A_h z - s_h on the held-out rows,
# d sse = 2 r' W A_h dz, so |d sse| / sse <= 2*||sqrt(W) A_h||_2 * ||dz||_2 / ||sqrt(W) r||_2 and ||dz||_2 <=
# sqrt(n)*max|z|*gap; the largest value of 2*||A_h||_2*sqrt(n)*max|z| / sqrt(sse) over the folds and lambdas of the
# oracle's own fits, as test_sparse_lasso_cv_host.test_cv_condition_factor printed it, rounded up
CV_CONDITION = 190.0  # 186.4


def cv_case(ap):
    """dict(D, A, s, foldid, lams, fold_lams (F x L, scale_lambda = 1))"""
    key = "cv"
    if key not in _CACHE:
        import scipy.sparse as sp
        A = R.matrix(ap, *CV_SHAPE)
        m, n = A.shape
        rng = np.random.default_rng(4646)
        xtrue = np.where(rng.random(n) < 0.3, rng.standard_normal(n), 0.0)
        s = A @ xtrue + 0.05 * rng.standard_normal(m)
        foldid = ap.solvers.cv_folds(m, CV_FOLDS, 0)
        lmax = float(np.max(np.abs(sp.csc_matrix(A).T @ s)))
        lams = lmax * np.logspace(0.0, -2.0, CV_NLAMBDA)
        train = np.array([float(np.sum(foldid != f)) for f in range(CV_FOLDS)])
        _CACHE[key] = dict(D=sp.csc_matrix(A), A=A, s=s, foldid=foldid, lams=lams,
                           fold_lams=(train / m)[:, None] * lams[None, :])
    return _CACHE[key]


def cv_oracle(ap, f, l):
    """the oracle's fit of fold f (CV_FOLDS: the full data) at lambda l of cv_case, from the zero start"""
    key = ("cv", f, l)
    if key not in _REFS:
        c = cv_case(ap)
        omega = (c["foldid"] != f).astype(np.float64)
        lam = float(c["fold_lams"][f, l]) if f < CV_FOLDS else float(c["lams"][l])
        _REFS[key] = oracle_run(c["A"], c["s"], omega, lam, R.loop_options(0))
    return _REFS[key]
