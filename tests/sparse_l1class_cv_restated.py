"""The sparse l1 classifier under held-out folds restated in NumPy (a helper of
test_sparse_l1class_cv_host / test_gpu_sparse_l1class_cv, not a test).  The reference of fit k is
sparse_l1class_restated.run on the FULL D with the weight vector weights o [fold != held_k]: the full-row problem with
zero-cost rows, which is the contract (a held-out row keeps its place in A = [D; I], in every norm and in both
tolerances).  The held-out sums come from D*z2 of that run, the cross-validation curve from cv_summary.

The problems: sparse_cases.problem's matrices (row 3 dense, row 5 and column 7 empty) at 257 x 65, 3 % and 80 x 200, 10 %
(fat), labels sign(A*truth + noise), F = 3 folds x L = 3 lambdas plus 3 full-data fits: 12 fits, two chunks of 10, so fold
fit 9 and the full-data fits 10 and 11 share the second chunk, and fit 9's twin 0 .. 8 the first.  Object "logistic": the logistic loss, no weights.  Object
"mixed": hinge and sqhinge in turn, observation weights and per-fit class costs.  Weights and class costs are multiples
of 1/8, so that every sum of costs is exact in any order: the held-out weight and the weighted errors are compared
exactly."""
import numpy as np
import scipy.sparse as sp

import l1class_restated as LR
import sparse_l1class_restated as R
import svm_cost_restated as SC
from sparse_reg_restated import relgap  # noqa: F401

# the largest relative gap between the CG restatement (sparse_l1class_restated.run) and the Cholesky restatement
# (l1class_restated.run), both at CG_TOL = 1e-14 on the zero-cost-row problem, over every run test_gpu_sparse_l1class_cv
# compares, every field and history entry, as test_sparse_l1class_cv_host printed it on the CPU:
#   per iteration (PARITY_LOOP), SHAPES x OBJECTS x 12 fits x nodualerror 0 | 1     2.688e-13 (257x65, logistic)
#   free-running (nodualerror = 1), SHAPES x 12 logistic fits                       8.294e-12 (80x200)
#   the edge folds, m = kScgRows + 1 and the sixteen fits of the cross-validation   7.813e-12
MEASURED_GAP = 8.3e-12  # 8.294e-12: a free-running logistic fit on 80x200
PARITY_BOUND = 10.0 * MEASURED_GAP  # the device's margin of q37 - q46: its summation order inside the products
assert PARITY_BOUND <= 1e-6
CG_TOL = R.CG_TOL

SHAPES = ((257, 65, 0.03), (80, 200, 0.10))
OBJECTS = ("logistic", "mixed")
F, L = 3, 3
K = (F + 1) * L
HELD = np.concatenate([np.repeat(np.arange(F), L), np.full(L, -1)])
FRACTIONS = (0.5, 0.2, 0.05)  # lambda_l / the full-data lambda_max of the object's first loss
PARITY_LOOP = dict(maxiters=12, domaxiters=1, objevals=1, rho=1.5)
FOLD_SEEDS = {(257, 65, 0.03): 0, (80, 200, 0.10): 0}  # chosen on the CPU: test_the_two_conditions_hold
FREE_DISTINCT = 3  # the nine free-running fold fits of the reference stop at >= this many distinct step counts
ROWS = 32  # kScgRows

# how far a relative gap g of zopt (against max|zopt|) can move a held-out loss sum S = sum_h c_i*phi(ell_i*t_i),
# t = D_h z2: phi is Lipschitz with constant lip_i (1 for logistic and hinge; 2*max(1 - q_i, 0), to first order, for
# sqhinge), so |dS| <= ||c_h o lip||_2 * ||D_h||_2 * ||dz2||_2 and ||dz2||_2 <= sqrt(n)*max|zopt|*g.  The largest
# ||c_h o lip||_2*||D_h||_2*sqrt(n)*max|zopt| / S over the reference's fits, as test_loss_sensitivity_factor printed it,
# rounded up
LOSS_CONDITION = 185.0  # 180.6

CV_SHAPE, CV_FOLDS, CV_NLAMBDA = (257, 65, 0.03), 3, 4
CV_SEED = 0
CV_LOOP = dict(nodualerror=1, objevals=1)

_CACHE, _REFS = {}, {}


def dyadic(rng, size, lo=4, hi=16):
    """multiples of 1/8 in [lo/8, hi/8]"""
    return rng.integers(lo, hi + 1, size).astype(np.float64) / 8.0


def case(ap, shape, obj, fold=None):
    """dict(D csc, A dense, ell, fold (m), held (K), fits (K of l1class_restated.Fit WITHOUT the fold mask: lambda,
    loss, weights, class cost), weights | None, classcost K x 2 | None, z0, u0); ``fold``: ids of its own (edge shapes)"""
    key = (tuple(shape), obj, None if fold is None else fold.tobytes())
    if key not in _CACHE:
        p = R.matrix(ap, *shape)
        A = np.asfortranarray(p["A"])
        m, n = A.shape
        rng = np.random.default_rng(4700 + m)
        score = A @ p["testx"]
        ell = np.where(score + 0.1 * float(np.std(score)) * rng.standard_normal(m) >= 0, 1.0, -1.0)
        fd = ap.solvers.cv_folds(m, F, FOLD_SEEDS.get(tuple(shape), 0)) if fold is None else np.asarray(fold)
        if obj == "mixed":
            weights = dyadic(rng, m)
            cc = np.ascontiguousarray(np.stack([dyadic(rng, K, 6, 12), dyadic(rng, K, 6, 12)], axis=1))
            losses = ["hinge" if k % 2 == 0 else "sqhinge" for k in range(K)]
        else:
            weights, cc, losses = None, None, ["logistic"] * K
        total = m if weights is None else float(weights.sum())
        w1 = np.ones(m) if weights is None else weights
        fits = []
        for k in range(K):
            f = LR.Fit(loss=losses[k], weights=weights, classcost=(1.0, 1.0) if cc is None else tuple(cc[k]))
            frac = 1.0 if HELD[k] < 0 else (total - float(w1[fd == HELD[k]].sum())) / total
            f.lam = FRACTIONS[k % L] * frac * LR.lambda_max(A, ell, f)
            fits.append(f)
        z0, u0 = (np.asfortranarray(0.1 * rng.standard_normal((m + n, K))) for _ in range(2))
        _CACHE[key] = dict(D=sp.csc_matrix(A), A=A, ell=ell, fold=fd, held=HELD.copy(), fits=fits, weights=weights,
                           classcost=cc, z0=z0, u0=u0, fold_key=key[2])
    return _CACHE[key]


def masked_fit(c, k):
    """fit k as the reference runs it: the weight vector weights o [fold != held_k]"""
    f = c["fits"][k]
    m = c["ell"].size
    w = (np.ones(m) if c["weights"] is None else c["weights"]) * (c["fold"] != c["held"][k])
    g = LR.Fit(loss=f.loss, lam=f.lam, weights=w, classcost=f.classcost)
    return g


def loop_options(c, k, loop, nodualerror, free):
    if free:
        return dict(loop or {}, objevals=1, nodualerror=nodualerror)
    return dict(loop, nodualerror=nodualerror, z0=c["z0"][:, k].copy(), u0=c["u0"][:, k].copy())


def restated_fit(ap, shape, obj, k, loop, nodualerror, free=False, fold=None, cholesky=False):
    c = case(ap, shape, obj, fold)
    key = (cholesky, tuple(shape), obj, c["fold_key"], k, nodualerror, free, tuple(sorted((loop or {}).items())))
    if key not in _REFS:
        o = loop_options(c, k, loop, nodualerror, free)
        if cholesky:
            _REFS[key] = LR.run(c["A"], c["ell"], masked_fit(c, k), o)
        else:
            _REFS[key] = R.run(c["D"], c["ell"], masked_fit(c, k), o)
    return _REFS[key]


def heldout_sums(A, ell, cost, loss, fold, held, zopt):
    """(loss, errors, weight, t on the held-out rows) of one fit at t = A*z2; cost: the UNMASKED c_i"""
    m = A.shape[0]
    rows = np.flatnonzero(fold == held) if held >= 0 else np.zeros(0, dtype=np.int64)
    t = A[rows] @ zopt[m:]
    q = ell[rows] * t
    c = cost[rows]
    return float(np.sum(c * SC.phi(q, loss))), float(np.sum(c[q <= 0.0])), float(np.sum(c)), t


def fit_sums(c, k, zopt):
    f = c["fits"][k]
    return heldout_sums(c["A"], c["ell"], f.cost(c["ell"]), f.loss, c["fold"], int(c["held"][k]), zopt)


def loss_condition(c, k, zopt):
    """the factor of LOSS_CONDITION for one fold fit (0 where the fit holds nothing out or the loss sum is 0)"""
    f = c["fits"][k]
    m, n = c["A"].shape
    rows = np.flatnonzero(c["fold"] == c["held"][k])
    if c["held"][k] < 0 or rows.size == 0:
        return 0.0
    S, _, _, t = fit_sums(c, k, zopt)
    q = c["ell"][rows] * t
    lip = 2.0 * np.maximum(1.0 - q, 0.0) if f.loss == "sqhinge" else np.ones(rows.size)
    cost = f.cost(c["ell"])[rows]
    if S == 0.0:
        return 0.0
    return float(np.linalg.norm(cost * lip) * np.linalg.norm(c["A"][rows], 2) * np.sqrt(n) * np.max(np.abs(zopt)) / S)


def error_margin(A, rows, ref, lam, rho, zbound):
    """what lets the weighted errors be compared exactly, on the reference run ``ref`` of a fit that holds ``rows`` out at
    lambda ``lam`` (no l1 weights, no ridge): the smaller of
      the smallest |t_i| - slack_i over the held-out rows whose t_i is not zero by structure, slack_i = zbound*||d_i||*
          max(||z2||, sqrt(n)*max|zopt|) (the z bound is relative to max|zopt| over the stacked vector), and
      the smallest | |x_j + u2_j| - lam/rho | - zbound*(max|xopt| + max|uopt|) over the coefficients: no coefficient is
          within the bound's reach of the soft threshold, so the support of z2 is the reference's.
    A row is zero by structure when every column it touches has z2_j = 0 (the empty row among them): with the support
    equal, t_i = +0.0 on both sides.  Positive: no sign, and no member of the support, is in doubt"""
    m = A.shape[0]
    zopt = np.asarray(ref["zopt"])
    z2 = zopt[m:]
    v = np.asarray(ref["xopt"]) + np.asarray(ref["uopt"])[m:]
    support = float(np.min(np.abs(np.abs(v) - lam / rho))) - zbound * float(np.max(np.abs(ref["xopt"])) +
                                                                            np.max(np.abs(ref["uopt"])))
    if len(rows) == 0:
        return support
    Ah = A[rows]
    t = Ah @ z2
    live = ((Ah != 0) & (z2 != 0)[None, :]).any(axis=1)
    if not live.any():
        return support
    slack = zbound * np.linalg.norm(Ah, axis=1) * max(np.sqrt(A.shape[1]) * np.max(np.abs(zopt)), np.linalg.norm(z2))
    return min(support, float(np.min(np.abs(t[live]) - slack[live])))


def fit_margin(c, k, ref, rho, zbound):
    rows = np.flatnonzero(c["fold"] == c["held"][k]) if c["held"][k] >= 0 else np.zeros(0, dtype=np.int64)
    return error_margin(c["A"], rows, ref, c["fits"][k].lam, rho, zbound)


# ---- the edge folds of test 3 (257 x 65): fold 1 is exactly the second row block, fold 2 the dense row 3 and the empty
# row 5, fold 3 is empty (nfolds = 4)
def edge_fold(m):
    fd = np.zeros(m, dtype=np.int64)
    fd[ROWS:2 * ROWS] = 1
    fd[[3, 5]] = 2
    return fd


EDGE_NFOLDS = 4
EDGE_HELD = np.array([1, 2, 3, -1, 0, 1, 2, 3, -1, 0, 1, 2])  # K = 12: every fold in both chunks
EDGE_M = (ROWS + 1, 65, 0.10)  # m = kScgRows + 1: one full row block and one row


def edge_problem(shape):
    """(shape, fold, held): the 257-row problem under edge_fold; m = kScgRows + 1 with the last row a fold of its own"""
    m = shape[0]
    if m > 2 * ROWS:
        return shape, edge_fold(m), EDGE_HELD
    return shape, (np.arange(m) >= ROWS).astype(np.int64), np.where(EDGE_HELD > 1, -1, EDGE_HELD)


def edge_case(ap, shape, fold, held):
    c = dict(case(ap, shape, "logistic", fold))
    c["held"] = np.asarray(held)
    c["fold_key"] = (c["fold_key"], tuple(int(h) for h in held))
    return c


def edge_fit(ap, c, k, cholesky=False):
    key = ("edge", cholesky, c["A"].shape, c["fold_key"], k)
    if key not in _REFS:
        o = loop_options(c, k, PARITY_LOOP, 0, False)
        run = LR.run if cholesky else R.run
        _REFS[key] = run(c["A"] if cholesky else c["D"], c["ell"], masked_fit(c, k), o)
    return _REFS[key]


# ---- the cross-validation of the last test
def cv_case(ap):
    """dict(D, A, ell, foldid, lams, fold_lams (F x L)) of l1classifier_cv on CV_SHAPE, logistic, no weights"""
    if "cv" not in _CACHE:
        c = case(ap, CV_SHAPE, "logistic")
        m = c["ell"].size
        foldid = ap.solvers.cv_folds(m, CV_FOLDS, CV_SEED)
        lmax = LR.lambda_max(c["A"], c["ell"], LR.Fit(loss="logistic"))
        lams = lmax * np.logspace(0.0, np.log10(0.05), CV_NLAMBDA)
        frac = np.array([(m - np.sum(foldid == f)) / m for f in range(CV_FOLDS)])
        _CACHE["cv"] = dict(D=c["D"], A=c["A"], ell=c["ell"], foldid=foldid, lams=lams, fold_lams=frac[:, None] * lams[None, :])
    return _CACHE["cv"]


def cv_fit(ap, f, l, cholesky=False):
    """fold f (CV_FOLDS: the full data) at lambda l, free-running under CV_LOOP"""
    key = ("cvfit", cholesky, f, l)
    if key not in _REFS:
        cv = cv_case(ap)
        m = cv["ell"].size
        lam = float(cv["fold_lams"][f, l]) if f < CV_FOLDS else float(cv["lams"][l])
        fit = LR.Fit(loss="logistic", lam=lam, weights=(cv["foldid"] != f).astype(np.float64))
        run = LR.run if cholesky else R.run
        _REFS[key] = run(cv["A"] if cholesky else cv["D"], cv["ell"], fit, dict(CV_LOOP))
    return _REFS[key]


def cv_sums(ap):
    """(loss, errors, weight) F x L of the restated fold fits"""
    cv = cv_case(ap)
    out = np.zeros((3, CV_FOLDS, CV_NLAMBDA))
    for f in range(CV_FOLDS):
        for l in range(CV_NLAMBDA):
            out[:, f, l] = heldout_sums(cv["A"], cv["ell"], np.ones(cv["ell"].size), "logistic", cv["foldid"], f,
                                        cv_fit(ap, f, l)["zopt"])[:3]
    return out
