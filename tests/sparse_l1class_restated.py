"""The sparse linear classifier with a matrix-free x-update restated in NumPy (a helper of test_sparse_l1class_host /
test_gpu_sparse_l1class, not a test): l1class_restated.run -- the oracle's admm() loop with A = [D; I_n],
B = -1, c = 0, z = [z1 (m); z2 (n)], stopcond 'standard', the z-prox and the objective of q42 -- whose x-update
(D'D + I)^-1 (D'(z1 - u1) + (z2 - u2)) is conjugate gradients on the shifted normal equations, the shift 1 whatever rho
is: the first solve of a run from 0, every later one from the previous x; a solve ends on ||r|| <= cg_tol*||y||, on
cg_maxit, on a zero right-hand side (x = 0) or on p.q = 0 (spmm_cg.hip's rules).  Every product goes through the
scipy.sparse matrix.

Also the problems of the sparse-classifier tests: sparse_cases.problem's matrices (row 3 dense, row 5 and column 7 empty,
unit columns), labels sign(A*truth + noise), and seven fits per problem.  The l1 weights, the observation weights and the
class costs are shared by an object, so the family fit runs in an object of its own, whose matrix has column 1 replaced
by ones (the unpenalised intercept: l1 weight 0)."""
import os

import numpy as np
import scipy.sparse as sp

import l1class_restated as LR
import penalty_restated as P
import svm_cost_restated as SC
from oracle import admm_ref
from sparse_reg_restated import relgap  # noqa: F401 (the measure of q37 - q41, over the same field names)

# the largest relative gap between this restatement and the Cholesky restatement (l1class_restated.run), both at CG_TOL,
# over every run that test_gpu_sparse_l1class compares with this restatement, every field and history entry, none
# excluded, computed on the CPU:
#   per iteration (PARITY_LOOP), SHAPES x MODES x seven fits x nodualerror 0 | 1    4.825e-13 (fit 3 on 600x120, per-fit)
#   free-running to the fit's own stop, nodualerror = 1, SHAPES x MODES x seven fits 1.923e-11 (fit 3 on 600x120, shared)
#   free-running to the fit's own stop, nodualerror = 0, SHAPES x MODES x seven fits 3.099e-09 (fit 0 on 257x65, shared
#       labels, 1000 iterations; 1.865e-09 on 80x200, 4.417e-10 on 600x120)
#   WIDE and TALL                                                                   2.713e-11 (the hinge fit on 60x8300)
#   the run at rho = 2.5 of the two-rho test (fit 2, 257x65 per-fit, 40 iterations) 5.126e-12
#   the K = 1 run against the dense object (fit 2, 257x65 shared, 220 steps)        7.613e-12
# (the two-chunk test compares bits between device runs only).  At the default cg_tol = 1e-12 the free-running fit 0
# under nodualerror = 0 reaches 2.4e-7 on 257x65 and 3.0e-7 on 80x200 -- its dual residual falls to 1e-6 of its start
# and the relative measure follows it down -- and 10x that lies outside 1e-6: hence CG_TOL = 1e-14 in these tests.
# The device's bound is 10x the largest (the margin of q37 - q41: its summation order inside the products)
MEASURED_GAP = 3.1e-9  # 3.099e-09: the logistic fit at 0.02*lambda_max on 257x65, shared labels, nodualerror = 0, 1000 iterations
PARITY_BOUND = 10.0 * MEASURED_GAP
assert PARITY_BOUND <= 1e-6  # never looser than the project's parity definition
CG_TOL = 1e-14  # of the restatement and of the device runs that are compared with it (the default is 1e-12)

SHAPES = ((600, 120, 0.05), (257, 65, 0.03), (80, 200, 0.10))  # the last one fat
SEEDS = {(600, 120, 0.05): 1, (257, 65, 0.03): 1, (80, 200, 0.10): 1}  # chosen on the CPU: see FREE_DISTINCT
MODES = ("shared", "perfit")  # one label column for every fit | one per fit
LOSSES = ("logistic", "logistic", "logistic", "logistic", "hinge", "sqhinge", "logistic")
FRACTIONS = (0.02, 0.1, 0.4, 1.25, 0.1, 0.1, 0.1)  # lambda_k / the fit's own lambda_max
K = len(FRACTIONS)
PLAIN = (0, 1, 2, 3, 4, 5)  # the fits of the object without weights
FAMILY = 6                  # logistic under shared l1 weights (0 on the ones column), a ridge, the sign constraint,
                            # observation weights and 'balanced' class costs: an object of its own
ONES_COLUMN = 1
PARITY_LOOP = dict(maxiters=12, domaxiters=1, objevals=1, rho=1.5)
FREE_DISTINCT = 4  # the seven free-running reference runs stop at >= this many distinct step counts
WIDE = (60, 8300, 0.02)   # more than 32 * 256 coefficients: a workgroup of the n-length kernels takes several row blocks
WIDE_FITS = (1, 4, 5)
WIDE_LOOP = dict(maxiters=10, domaxiters=1, objevals=1)
TALL = (8200, 40, 0.02)   # more than 32 * 256 rows: a workgroup of the row kernel takes several row blocks
TALL_FITS = (0, 4, 5)
TALL_LOOP = dict(maxiters=10, domaxiters=1, objevals=1)


class CgUnitShift:
    """CG on (D'D + I) x = y with the solver's state: x of the previous solve, inner iterations, capped solves"""

    def __init__(self, D, cg_tol=CG_TOL, cg_maxit=200):
        self.D, self.Dt = sp.csr_matrix(D), sp.csr_matrix(D.T)
        self.tol, self.maxit = float(cg_tol), int(cg_maxit)
        self.x, self.total, self.capped = None, 0, 0

    def op(self, v):
        return self.Dt @ (self.D @ v) + v

    def solve(self, y):
        n = y.size
        if self.x is None:
            x, r = np.zeros(n), y.copy()
        else:
            x = self.x.copy()
            r = y - self.op(x)
        yy, rs = float(y @ y), float(r @ r)
        if yy == 0.0:
            self.x = np.zeros(n)
            return self.x.copy()
        ynorm = np.sqrt(yy)
        p = r.copy()
        it, converged = 0, np.sqrt(rs) <= self.tol * ynorm
        while not converged and it < self.maxit:
            q = self.op(p)
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


def run(D, ell, fit, options=None, cg_tol=CG_TOL, cg_maxit=200):
    """l1class_restated.run on a scipy.sparse D with the x-update above; the results of the oracle's admm() plus
    cg_iters_total and cg_capped_updates"""
    options = dict(options or {})
    D = sp.csr_matrix(D)
    Dt = sp.csr_matrix(D.T)
    m, n = D.shape
    ell = np.asarray(ell, dtype=np.float64).reshape(-1)
    cost = fit.cost(ell)
    cg = CgUnitShift(D, cg_tol, cg_maxit)
    A = sp.vstack([D, sp.identity(n, format="csr")], format="csr")

    def xminf(_x, z, u, _rho):
        t = z - u
        return cg.solve(Dt @ t[:m] + t[m:])

    def zming(x, _z, u, rho):
        z1 = SC.prox(D @ x + u[:m], ell, (fit.C * cost) / rho, fit.loss)
        z2 = P.prox(x + u[m:], fit.pen, fit.lam / rho, 0.0, rho)
        return np.concatenate([z1, z2])

    def obj(x, z):
        w = 1.0 if fit.pen.w is None else fit.pen.w
        z2 = z[m:]
        return (fit.C * float(np.sum(cost * SC.phi(ell * (D @ x), fit.loss))) + fit.lam * float(np.sum(w * np.abs(z2)))
                + 0.5 * fit.pen.ridge * float(z2 @ z2))

    options.update(A=A, B=-1, c=0, m=m + n, nB=m + n, stopcond="standard", obj=obj)
    options.setdefault("x0", np.zeros(n))
    res = admm_ref.admm(xminf, zming, options)
    res["cg_iters_total"], res["cg_capped_updates"] = cg.total, cg.capped
    return res


# ---- the problems
_CACHE = {}
_REFS = {}


def matrix(ap, rows, cols, density):
    from sparse_cases import problem as lasso_problem
    return lasso_problem(ap, rows, cols, density, seed=SEEDS.get((rows, cols, density), 3))


def case(ap, shape, mode):
    """dict(D csc_matrix, A dense, Dw / Aw the family object's matrix, ELL m x 1 | m x K, fits (K of
    l1class_restated.Fit, lambda set), z0, u0 (m + n) x K) of one (shape, mode)"""
    key = (tuple(shape), mode)
    if key not in _CACHE:
        p = matrix(ap, *shape)
        A = np.asfortranarray(p["A"])
        m, n = A.shape
        rng = np.random.default_rng(SEEDS.get(tuple(shape), 3) + 4300)
        score = A @ p["testx"]
        noise = 0.1 * float(np.std(score))
        cols = K if mode == "perfit" else 1
        ELL = np.empty((m, cols), order="F")
        for k in range(cols):
            truth = p["testx"] * (1.0 + 0.3 * rng.standard_normal(n) * (k > 0))
            ELL[:, k] = np.where(A @ truth + noise * rng.standard_normal(m) >= 0, 1.0, -1.0)
        Aw = A.copy(order="F")
        Aw[:, ONES_COLUMN] = 1.0
        lw = rng.uniform(0.5, 2.0, n)
        lw[ONES_COLUMN] = 0.0  # the intercept is not penalised
        weights = rng.uniform(0.5, 2.0, m)
        fits = []
        for k in range(K):
            if k == FAMILY:
                f = LR.Fit(loss=LOSSES[k], ridge=0.5, nonnegative=1, l1weights=lw, weights=weights, classcost="balanced")
            else:
                f = LR.Fit(loss=LOSSES[k])
            f.lam = FRACTIONS[k] * LR.lambda_max(Aw if k == FAMILY else A, label(ELL, k), f)
            fits.append(f)
        z0, u0 = (np.asfortranarray(0.1 * rng.standard_normal((m + n, K))) for _ in range(2))
        _CACHE[key] = dict(D=sp.csc_matrix(A), A=A, Dw=sp.csc_matrix(Aw), Aw=Aw, ELL=ELL, fits=fits, z0=z0, u0=u0)
    return _CACHE[key]


def label(ELL, k):
    return np.ascontiguousarray(ELL[:, k if ELL.shape[1] > 1 else 0])


def fit_options(c, k, loop, nodualerror):
    return dict(loop, nodualerror=nodualerror, z0=c["z0"][:, k].copy(), u0=c["u0"][:, k].copy())


def free_options(loop, nodualerror):
    """a free-running run at the default tolerances from the zero start; loop: maxiters, if any"""
    return dict(loop or {}, objevals=1, nodualerror=nodualerror)


def restated_fit(ap, shape, mode, k, loop, nodualerror, free=False):
    """the CG restatement's run of fit k of (shape, mode), computed once"""
    key = ("cg", tuple(shape), mode, k, nodualerror, free, tuple(sorted((loop or {}).items())))
    if key not in _REFS:
        c = case(ap, shape, mode)
        o = free_options(loop, nodualerror) if free else fit_options(c, k, loop, nodualerror)
        _REFS[key] = run(c["Dw"] if k == FAMILY else c["D"], label(c["ELL"], k), c["fits"][k], o)
    return _REFS[key]


def cholesky_fit(ap, shape, mode, k, loop, nodualerror, free=False):
    """the same run of l1class_restated.run (a SciPy Cholesky of D'D + I), computed once"""
    key = ("chol", tuple(shape), mode, k, nodualerror, free, tuple(sorted((loop or {}).items())))
    if key not in _REFS:
        c = case(ap, shape, mode)
        o = free_options(loop, nodualerror) if free else fit_options(c, k, loop, nodualerror)
        _REFS[key] = LR.run(c["Aw"] if k == FAMILY else c["A"], label(c["ELL"], k), c["fits"][k], o)
    return _REFS[key]



# ---- the free-running references under nodualerror = 0, recorded
# Under the default stop rule on both residuals the hinge fit and the two small-lambda fits take all 1000 iterations, and
# the seven runs of one (shape, mode) cost this restatement 15 - 25 s of CPU time: too long for a test that every later
# change runs again.  They are computed once (record_free_dual) and kept under tests/golden/sparse_l1class (a folder of
# its own: tests/golden/*.npz are the oracle's fixtures, which test_golden enumerates); test_sparse_l1class_host
# recomputes the two cheapest fits of every file and holds them against the record.
RECORDED = ("xopt", "zopt", "uopt", "pnorm", "perr", "dnorm", "derr", "objevals", "objopt", "steps", "cg_iters_total",
            "cg_capped_updates")


def recorded_path(shape, mode):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_l1class",
                        f"free_dual_{shape[0]}x{shape[1]}_{mode}.npz")


def recorded_free_dual(shape, mode):
    """the K runs restated_fit(ap, shape, mode, k, None, 0, free=True) as record_free_dual wrote them"""
    with np.load(recorded_path(shape, mode)) as f:
        runs = [{key: f[f"fit{k}_{key}"] for key in RECORDED} for k in range(K)]
    for r in runs:
        for key in ("steps", "cg_iters_total", "cg_capped_updates"):
            r[key] = int(r[key])
        r["objopt"] = float(r["objopt"])
    return runs


def record_free_dual(ap, shape, mode):
    """(by hand, when a problem or CG_TOL changes) python -c "import admm_project_amd as ap, sparse_l1class_restated as R;
    [R.record_free_dual(ap, s, m) for s in R.SHAPES for m in R.MODES]" from tests/, the repository root on sys.path"""
    out = {}
    for k in range(K):
        r = restated_fit(ap, shape, mode, k, None, 0, free=True)
        out.update({f"fit{k}_{key}": np.asarray(r[key]) for key in RECORDED})
    np.savez_compressed(recorded_path(shape, mode), **out)
