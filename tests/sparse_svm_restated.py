"""The linear SVM with a matrix-free x-update restated in NumPy (a helper of test_sparse_svm_host / test_gpu_sparse_svm,
not a test): the loop of oracle.solvers_ref.linearsvm -- the oracle's admm() with the operators and
options unwrappedadmm.m:76-92 sets up -- whose x-update D^+(z - u) is conjugate gradients on D'D x = D'(z - u): the first
solve of a run starts from 0 (the reference's x-update never reads x0), every later one from the previous x; a solve
ends on ||r|| <= cg_tol*||y||, on cg_maxit, on a zero right-hand side (x = 0) or on p.q = 0, the last two without a
division.  The z-prox and the objective are svm_cost_restated's (every loss, costs optional).

Also the problems of the sparse-SVM tests: sparse_cases.problem's matrices with labels from planted directions."""
import numpy as np

import svm_cost_restated as SC
from oracle import admm_ref

FIELDS = ("xopt", "zopt", "uopt", "pnorm", "perr", "Hnormsq", "objevals", "objopt")


class CgPinv:
    """x-update closure with the solver's state: x of the previous solve, inner iterations, capped solves"""

    def __init__(self, D, cg_tol=1e-12, cg_maxit=200):
        self.D, self.tol, self.maxit = D, float(cg_tol), int(cg_maxit)
        self.x, self.total, self.capped = None, 0, 0

    def __call__(self, _x, z, u, _rho):
        D = self.D
        y = D.T @ (z - u)
        if self.x is None:
            x, r = np.zeros(D.shape[1]), y.copy()
        else:
            x = self.x.copy()
            r = y - D.T @ (D @ x)
        yy, rs = float(y @ y), float(r @ r)
        if yy == 0.0:
            self.x = np.zeros(D.shape[1])
            return self.x.copy()
        ynorm = np.sqrt(yy)
        p = r.copy()
        it, converged = 0, np.sqrt(rs) <= self.tol * ynorm
        while not converged and it < self.maxit:
            q = D.T @ (D @ p)
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


def run(D, ell, C, loss, options=None, cost=None, cg_tol=1e-12, cg_maxit=200):
    """one class: results of the oracle's admm() plus cg_iters_total and cg_capped_updates"""
    D = np.asarray(D, dtype=np.float64)
    ell = np.asarray(ell, dtype=np.float64)
    cost = np.ones(ell.size) if cost is None else np.asarray(cost, dtype=np.float64)
    ploss = loss if loss in SC.LOSSES else "hinge"
    m = D.shape[0]
    xmin = CgPinv(D, cg_tol, cg_maxit)
    o = dict(options or {})
    o.update(A=D, At=D.T, B=-1, nB=m, c=0, m=m, maxiters=1000, stopcond="both", nodualerror=1,
             obj=lambda x, z: SC.objective(D, ell, C, cost, x, loss))
    res = admm_ref.admm(xmin, lambda x, _z, u, rho: SC.prox(D @ x + u, ell, (C * cost) / rho, ploss), o)
    res["cg_iters_total"], res["cg_capped_updates"] = xmin.total, xmin.capped
    return res


def oracle_run(D, ell, C, loss, options, cost=None):
    """the reference side of the parity tests: oracle.solvers_ref.linearsvm where the oracle has the loss ('hinge', '01'
    without costs), else the oracle's unwrappedadmm (dense pinv) with the restated prox (svm_cost_restated.run)"""
    from oracle import solvers_ref as S
    if cost is None and loss in ("hinge", "01"):
        return S.linearsvm(D, ell, C, dict(options, lossfunction=loss))
    return SC.run(D, ell, C, np.ones(len(ell)) if cost is None else cost, loss, dict(options))


def relgap(got, ref, steps=None):
    """the largest relative gap over FIELDS, by test_gpu_svm_ovr's measure: scalar histories per entry against
    max(|ref|, 1e-12 + 1e-3 max|ref|), everything else against max|ref|"""
    worst = 0.0
    for key in FIELDS:
        if key not in ref:
            continue
        a, b = np.atleast_1d(np.asarray(got[key], dtype=np.float64)), np.atleast_1d(np.asarray(ref[key], dtype=np.float64))
        if steps is not None and key in ("pnorm", "perr", "Hnormsq", "objevals"):
            a, b = a[:steps], b[:steps]
        assert a.shape == b.shape, (key, a.shape, b.shape)
        if b.ndim == 1 and not key.endswith("opt"):
            err = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-12 + 1e-3 * np.max(np.abs(b)))))
        else:
            err = float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))
        worst = max(worst, err)
    return worst


# ---- the problems
SHAPES = ((600, 120, 0.05), (257, 65, 0.03))
LOSSES3 = ("hinge", "logistic", "sqhinge")
SEEDS = {(600, 120, 0.05): 3, (257, 65, 0.03): 3}  # chosen on the CPU: the three classes' oracle runs stop at different steps
_CACHE = {}


def problem(ap, rows, cols, density, K=3):
    """sparse_cases.problem's matrix (row 3 dense, row 5 and column 7 empty, unit columns) with K label columns from
    planted directions and per-class starts: dict(D csc_matrix, A dense, labels, ELL m x K, C, x0, z0, u0)"""
    key = (rows, cols, density, K)
    if key not in _CACHE:
        from sparse_cases import problem as lasso_problem
        seed = SEEDS[(rows, cols, density)]
        p = lasso_problem(ap, rows, cols, density, seed=seed)
        rng = np.random.default_rng(seed + 977)
        W = rng.standard_normal((cols, K))
        labels = np.argmax(p["A"] @ W + 0.05 * rng.standard_normal((rows, K)), axis=1).astype(np.float64)
        ELL = np.asfortranarray(np.where(labels[:, None] == np.arange(K)[None, :], 1.0, -1.0))
        x0, z0, u0 = (np.asfortranarray(rng.random((r, K))) for r in (cols, rows, rows))
        _CACHE[key] = dict(D=p["D"], A=p["A"], labels=labels, ELL=ELL, C=1.0, x0=x0, z0=z0, u0=u0)
    return _CACHE[key]


_REFS = {}


def oracle_class(ap, shape, c, loss, K=3, label=None):
    """the oracle's run of class c (labels `label`, default c) with loss `loss`, computed once"""
    key = (shape, c, loss, K, label)
    if key not in _REFS:
        p = problem(ap, *shape, K=K)
        ell = np.where(p["labels"] == (c if label is None else label), 1.0, -1.0)
        _REFS[key] = oracle_run(p["A"], ell, p["C"], loss, dict(objevals=1, x0=p["x0"][:, c], z0=p["z0"][:, c],
                                                                u0=p["u0"][:, c]))
    return _REFS[key]
