"""The group and sparse-group penalty on the sparse linear classifiers restated in NumPy (a helper of
test_group_l1class_host / test_gpu_group_l1class, not a test): l1class_restated.run -- the oracle's admm() loop with
A = [D; I_n], B = -1, c = 0, z = [z1 (m); z2 (n)], stopcond 'standard' -- with ONE change, the z2-update

    z2 = penalty_restated.prox(x + u2, pen, pen.lambda1(lam)/rho, lam/rho, rho)

and the objective's penalty through penalty_restated.g_of.  Per fit

    minimise C*sum_i c_i*phi(ell_i*(D*x)_i) + lambda*sum_g omega_g*||x_g|| + l1*sum_j w_j*|x_j| + mu/2*||x||^2  [x >= 0]

The x-update is a SciPy Cholesky of D'D + I (xsolve = 'chol': the reference of the dense object, and what the CG form is
measured against) or sparse_l1class_restated.CgUnitShift at its CG_TOL (xsolve = 'cg': the reference of the sparse object).
``kkt`` returns the worst violation of the group lasso's optimality conditions (l1 = 0, smooth losses), which is how
test_group_l1class_host trusts all of it.

The problems: dense 300 x 70 and the fat 60 x 130 (l1class_restated.problem's matrices), sparse (257, 65, 0.03) and the fat
(80, 200, 0.10) (sparse_l1class_restated.matrix), each with column 0 replaced by ones -- the intercept, a group of one
with omega = 0 -- and q41's groups 1, 20, 40, then nines (group_multi_restated.sizes_for); WIDE (60, 8300, 0.02) with
groups of 7 and one group of 300, every group penalised.  Seven fits: logistic pure-group at four fractions of the fit's
group lambda_max, a hinge and a squared-hinge fit, and a sparse-group logistic fit under l1 weights, a ridge term and the
sign constraint.  The l1 weights are shared by an object, so the last fit runs in an object of its own."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import l1class_restated as LR
import penalty_restated as P
import svm_cost_restated as SC
from group_multi_restated import sizes_for
from oracle import admm_ref
from sparse_l1class_restated import CG_TOL, WIDE, CgUnitShift, matrix
from sparse_reg_restated import relgap  # noqa: F401

# The largest relative gap (relgap: every field and history entry) between the CG restatement and the Cholesky one, both
# at cg_tol = 1e-14, over every run test_gpu_group_l1class compares on the sparse object, as
# test_group_l1class_host.test_cg_restatement_against_cholesky_measures_the_gap printed it on the CPU:
#   forced 12 iterations, SPARSE_SHAPES x seven fits x nodualerror 0 | 1          1.089e-12
#   free-running (nodualerror = 1), SPARSE_SHAPES[0] x seven fits                 1.803e-12
#   WIDE, 10 forced iterations, WIDE_FITS                                         below that
#   the masked-weight runs of the folds test and the fits of the cross-validation 1.926e-12
MEASURED_GAP = 2.0e-12  # 1.926e-12
PARITY_BOUND = 10.0 * MEASURED_GAP  # the device's margin of q37 - q47: its summation order inside the products
assert PARITY_BOUND <= 1e-6
DENSE_BOUND = 1e-6  # the project's parity definition (test_gpu_l1class.BOUND)

DENSE_SHAPES = ((300, 70), (60, 130))
SPARSE_SHAPES = ((257, 65, 0.03), (80, 200, 0.10))
LOSSES = ("logistic", "logistic", "logistic", "logistic", "hinge", "sqhinge", "logistic")
FRACTIONS = (0.05, 0.15, 0.35, 1.25, 0.3, 0.2, 0.25)  # lambda_k / the fit's own group lambda_max
L1_FRACTION = 0.05  # the family fit's l1 / its l1classifier lambda_max
K = len(FRACTIONS)
PLAIN = (0, 1, 2, 3, 4, 5)
FAMILY = 6
PARITY_LOOP = dict(maxiters=12, domaxiters=1, objevals=1, rho=1.5)
FREE_DISTINCT = 4
WIDE_FITS = (1, 4, 5)
WIDE_LOOP = dict(maxiters=10, domaxiters=1, objevals=1)
WIDE_SIZES = [7] * 571 + [300] + [7] * 571 + [6]
assert sum(WIDE_SIZES) == WIDE[1]
SEEDS = {}  # per shape, chosen on the CPU so that the reference holds test_group_l1class_host's conditions

# the cross-validation of the last GPU test: F = 3 folds x L = 3 lambdas on (257, 65, 0.03), logistic, free-running
CV_SHAPE, CV_FOLDS, CV_NLAMBDA, CV_SEED = SPARSE_SHAPES[0], 3, 3, 0
CV_LOOP = dict(nodualerror=1, objevals=1)
CV_FRACTIONS = (0.5, 0.2, 0.08)
# sparse_l1class_cv_restated.LOSS_CONDITION's measure on the fold fits of this cross-validation (how far a relative gap of
# zopt can move a held-out loss sum), as test_group_l1class_host.test_cv_loss_condition printed it, rounded up
LOSS_CONDITION = 270.0  # 267.1


class Fit(LR.Fit):
    """l1class_restated.Fit with the groups: lam is the group strength, l1 the l1 strength"""

    def __init__(self, sizes, groupweights=None, l1=0.0, **kw):
        super().__init__(**kw)
        self.pen = P.Penalty(l1weights=kw.get("l1weights"), ridge=kw.get("ridge", 0.0), nonnegative=kw.get("nonnegative", 0),
                             sizes=sizes, groupweights=groupweights, l1=l1)


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def lambda_max(D, ell, fit):
    """C*|phi'(0)|*max over omega_g > 0 of ||(D'(c o ell))_g||_2 / omega_g"""
    g = np.asarray(D.T @ (fit.cost(ell) * ell)).reshape(-1)
    off = offsets(fit.pen.sizes)
    gw = np.ones(len(fit.pen.sizes)) if fit.pen.gw is None else fit.pen.gw
    return fit.C * LR.SLOPE0[fit.loss] * max(float(np.linalg.norm(g[off[j]:off[j + 1]])) / gw[j]
                                              for j in range(len(gw)) if gw[j] > 0)


def run(D, ell, fit, options=None, xsolve="chol", cg_tol=CG_TOL, cg_maxit=200):
    """l1class_restated.run (xsolve = 'chol') or sparse_l1class_restated.run (xsolve = 'cg') with the grouped z2-update"""
    options = dict(options or {})
    ell = np.asarray(ell, dtype=np.float64).reshape(-1)
    cost = fit.cost(ell)
    if xsolve == "cg":
        Dm = sp.csr_matrix(D)
        Dt = sp.csr_matrix(Dm.T)
        n = Dm.shape[1]
        cg = CgUnitShift(Dm, cg_tol, cg_maxit)
        solve = cg.solve
        A = sp.vstack([Dm, sp.identity(n, format="csr")], format="csr")
    else:
        Dm = D.toarray() if sp.issparse(D) else np.asarray(D)
        Dt = Dm.T
        n = Dm.shape[1]
        F = sla.cho_factor(Dm.T @ Dm + np.eye(n), lower=True)
        solve = lambda y: sla.cho_solve(F, y)
        A = np.vstack([Dm, np.eye(n)])
    m = Dm.shape[0]

    def xminf(_x, z, u, _rho):
        t = z - u
        return solve(Dt @ t[:m] + t[m:])

    def zming(x, _z, u, rho):
        z1 = SC.prox(Dm @ x + u[:m], ell, (fit.C * cost) / rho, fit.loss)
        z2 = P.prox(x + u[m:], fit.pen, fit.pen.lambda1(fit.lam) / rho, fit.lam / rho, rho)
        return np.concatenate([z1, z2])

    def obj(x, z):
        return fit.C * float(np.sum(cost * SC.phi(ell * (Dm @ x), fit.loss))) + P.g_of(z[m:], fit.pen, fit.lam)

    options.update(A=A, B=-1, c=0, m=m + n, nB=m + n, stopcond="standard", obj=obj)
    options.setdefault("x0", np.zeros(n))
    return admm_ref.admm(xminf, zming, options)


def kkt(D, ell, fit, x):
    """the worst violation of  ||(g + mu*x)_g|| <= lambda*omega_g on a zero group  and  (g + mu*x)_g = -lambda*omega_g*
    x_g/||x_g|| elsewhere, g = C*D'(c.*ell.*phi'(ell.*D*x)); l1 = 0 and a smooth loss"""
    assert fit.pen.l1 == 0.0 and not fit.pen.nonnegative and fit.loss != "hinge"
    ell = np.asarray(ell, dtype=np.float64).reshape(-1)
    g = fit.C * (D.T @ (fit.cost(ell) * ell * LR.dphi(ell * (D @ x), fit.loss))) + fit.pen.ridge * x
    off = offsets(fit.pen.sizes)
    gw = np.ones(len(fit.pen.sizes)) if fit.pen.gw is None else fit.pen.gw
    worst = 0.0
    for j in range(len(gw)):
        xg, gg = x[off[j]:off[j + 1]], g[off[j]:off[j + 1]]
        nx = float(np.linalg.norm(xg))
        if nx == 0.0:
            v = max(float(np.linalg.norm(gg)) - fit.lam * gw[j], 0.0)
        else:
            v = float(np.max(np.abs(gg + fit.lam * gw[j] * xg / nx)))
        worst = max(worst, v)
    return worst


# ---- the problems
_CACHE, _REFS = {}, {}


def _labels(A, sizes, rng, intercept):
    """labels from a group-sparse truth: every third group of the penalised ones is live"""
    n = A.shape[1]
    off = offsets(sizes)
    truth = np.zeros(n)
    for j in range(1 if intercept else 0, len(sizes), 3):
        truth[off[j]:off[j + 1]] = rng.standard_normal(sizes[j]) * 2.0
    if intercept:
        truth[0] = 0.3
    score = A @ truth
    return np.where(score + 0.1 * float(np.std(score)) * rng.standard_normal(A.shape[0]) >= 0, 1.0, -1.0)


def case(ap, shape):
    """dict(kind 'dense' | 'sparse', A dense, D (the matrix the device gets), ell, sizes, gw, lw (the family's l1
    weights), fits (K of Fit, lambda and l1 set), z0, u0 (m + n) x K) of one shape; WIDE has no intercept"""
    key = tuple(shape)
    if key not in _CACHE:
        dense = len(shape) == 2
        wide = key == tuple(WIDE)
        rng = np.random.default_rng(4800 + SEEDS.get(key, 0))
        A = np.array(LR.problem(shape, seed=SEEDS.get(key, 0))["D"] if dense else matrix(ap, *shape)["A"], order="F")
        m, n = A.shape
        if not wide:
            A[:, 0] = 1.0
        sizes = list(WIDE_SIZES) if wide else sizes_for(n)
        gw = np.sqrt(np.asarray(sizes, dtype=np.float64))
        if not wide:
            gw[0] = 0.0  # the intercept is not penalised
        ell = _labels(A, sizes, rng, not wide)
        lw = rng.uniform(0.5, 2.0, n)
        lw[0] = 0.0
        fits = []
        for k in range(K):
            if k == FAMILY:
                f = Fit(sizes, gw, loss=LOSSES[k], ridge=0.5, nonnegative=1, l1weights=lw)
                f.pen.l1 = L1_FRACTION * LR.lambda_max(A, ell, LR.Fit(loss=LOSSES[k], l1weights=lw))
            else:
                f = Fit(sizes, gw, loss=LOSSES[k])
            f.lam = FRACTIONS[k] * lambda_max(A, ell, f)
            fits.append(f)
        z0, u0 = (np.asfortranarray(0.1 * rng.standard_normal((m + n, K))) for _ in range(2))
        _CACHE[key] = dict(kind="dense" if dense else "sparse", A=A, D=A if dense else sp.csc_matrix(A), ell=ell,
                           sizes=np.asarray(sizes, dtype=np.int64), gw=gw, lw=lw, fits=fits, z0=z0, u0=u0)
    return _CACHE[key]


def loop_options(c, k, loop, nodualerror, free):
    if free:
        return dict(loop or {}, objevals=1, nodualerror=nodualerror)
    return dict(loop, nodualerror=nodualerror, z0=c["z0"][:, k].copy(), u0=c["u0"][:, k].copy())


def reference_fit(ap, shape, k, loop, nodualerror, free=False, xsolve=None, weights=None):
    """fit k of a shape, computed once: by default with the x-update of the object that runs the shape (Cholesky for a
    dense D, CG for a sparse one); ``weights``: observation weights of the run (the masked vector of the folds test)"""
    c = case(ap, shape)
    xsolve = xsolve or ("chol" if c["kind"] == "dense" else "cg")
    key = (tuple(shape), k, nodualerror, free, xsolve, tuple(sorted((loop or {}).items())),
           None if weights is None else weights.tobytes())
    if key not in _REFS:
        f = c["fits"][k]
        if weights is not None:
            g = Fit(f.pen.sizes, f.pen.gw, l1=f.pen.l1, loss=f.loss, lam=f.lam, ridge=f.pen.ridge,
                    nonnegative=f.pen.nonnegative, l1weights=f.pen.w, weights=weights)
            f = g
        _REFS[key] = run(c["A"], c["ell"], f, loop_options(c, k, loop, nodualerror, free), xsolve=xsolve)
    return _REFS[key]


def device_options(c, cols, loop, nodualerror, starts=True, **more):
    """the options of groupclassifier_multi for the fits ``cols`` of a case -- fits of PLAIN, or [FAMILY] alone under the
    shared l1 weights -- and their lambdas"""
    cols = list(cols)
    fits = [c["fits"][k] for k in cols]
    family = cols == [FAMILY]
    assert family or FAMILY not in cols
    o = dict(loop or {})
    o.update(lossfunction=[f.loss for f in fits], ridge=[f.pen.ridge for f in fits],
             nonnegative=[f.pen.nonnegative for f in fits], l1=[f.pen.l1 for f in fits], groupweights=c["gw"],
             nodualerror=nodualerror)
    if family:
        o["l1weights"] = c["lw"]
    if c["kind"] == "sparse":
        o["cg_tol"] = CG_TOL
    if starts:
        o.update(z0=np.asfortranarray(c["z0"][:, cols]), u0=np.asfortranarray(c["u0"][:, cols]))
    o.update(more)
    return o, [f.lam for f in fits]


def threshold_margin(c, k, ref, rho):
    """the smallest relative distance | ||e_g|| - t_g | / max(||e_g||, t_g) over the penalised groups at the reference's
    last z2-update, e = stage 1 at x + u2 of the LAST iterate -- (xopt + uopt's block is v of the next update; the
    support of zopt was decided one update earlier by the same quantities to within the step's change, so both are
    held) -- t_g = (lam/rho)*omega_g.  Large against the parity bound: no group's membership is in doubt"""
    f = c["fits"][k]
    m = c["A"].shape[0]
    v = np.asarray(ref["xopt"]) + np.asarray(ref["uopt"])[m:]
    w = np.ones(v.size) if f.pen.w is None else f.pen.w
    e = P.soft(v, (f.pen.l1 / rho) * w, f.pen.nonnegative)
    off = offsets(f.pen.sizes)
    worst = np.inf
    for j in range(len(f.pen.sizes)):
        t = (f.lam / rho) * f.pen.gw[j]
        if t == 0.0:
            continue
        ne = float(np.linalg.norm(e[off[j]:off[j + 1]]))
        worst = min(worst, abs(ne - t) / max(ne, t))
    return worst


def groups_alive(z2, sizes):
    off = offsets(sizes)
    return np.array([bool(np.any(z2[off[j]:off[j + 1]] != 0)) for j in range(len(sizes))])


# ---- the cross-validation
def cv_case(ap):
    """dict(D, A, ell, sizes, gw, foldid, lams, fold_lams (F x L)) of groupclassifier_cv on CV_SHAPE, logistic"""
    if "cv" not in _CACHE:
        c = case(ap, CV_SHAPE)
        m = c["ell"].size
        foldid = ap.solvers.cv_folds(m, CV_FOLDS, CV_SEED)
        lmax = lambda_max(c["A"], c["ell"], c["fits"][0])
        lams = lmax * np.asarray(CV_FRACTIONS)
        frac = np.array([(m - np.sum(foldid == f)) / m for f in range(CV_FOLDS)])
        _CACHE["cv"] = dict(c, foldid=foldid, lams=lams, fold_lams=frac[:, None] * lams[None, :])
    return _CACHE["cv"]


def cv_fit(ap, f, l, xsolve="cg"):
    """fold f (CV_FOLDS: the full data) at lambda l, free-running under CV_LOOP"""
    key = ("cvfit", xsolve, f, l)
    if key not in _REFS:
        cv = cv_case(ap)
        lam = float(cv["fold_lams"][f, l]) if f < CV_FOLDS else float(cv["lams"][l])
        fit = Fit(cv["sizes"], cv["gw"], loss="logistic", lam=lam, weights=(cv["foldid"] != f).astype(np.float64))
        _REFS[key] = run(cv["A"], cv["ell"], fit, dict(CV_LOOP), xsolve=xsolve)
    return _REFS[key]
