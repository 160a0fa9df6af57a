"""The grouped multi-fit lasso restated in NumPy (a helper of test_grouplasso_multi_host / test_gpu_grouplasso_multi, not a
test): the oracle's admm() loop with the operators and options lasso.m:227-239 sets up (A = 1, B = -1,
c = 0, sizes n, stopcond 'standard'), the z-prox and objective of penalty_restated with groups in force, and as x-update
what each object applies -- the EXPLICIT inverse of D'D + rho*I (lasso_multi_restated.InverseSolve, the dense object) or
conjugate gradients on the shifted normal equations at cg_tol = 1e-12 (sparse_lasso_restated.CgShift, the sparse object).
The reference of the parity tests is penalty_restated.run (Cholesky solves) per fit.

The problems are the existing ones: lasso_multi_restated.SHAPES (dense) and sparse_lasso_restated.SHAPES (sparse) with
their matrices, responses, l1 weights and starts; what is new is the groups and the grid of seven fits."""
import numpy as np

import lasso_multi_restated as LM
import penalty_restated as PR
import sparse_lasso_restated as SL
from oracle import admm_ref
from sparse_reg_restated import relgap  # noqa: F401 (the measure of q37 - q40, over the same field names)

KINDS = ("dense", "sparse")
SHAPES = dict(dense=LM.SHAPES, sparse=SL.SHAPES)
MODES = SL.MODES
RHO = 1.0
# lambda_k as a fraction of the fit's own group lambda_max = max_g ||(D's_k)_g|| / omega_g: five pure group fits, one of
# them above lambda_max (z = 0 exactly), a sparse-group fit, and a fit with l1 under the shared l1 weights, a ridge term
# and the sign constraint.  l1_k is a fraction of ||D's_k||_inf.
FRACTIONS = (0.05, 0.15, 0.35, 0.7, 1.25, 0.25, 0.2)
L1_FRACTIONS = (0.0, 0.0, 0.0, 0.0, 0.0, 0.05, 0.1)
RIDGE = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5)
NONNEG = (0, 0, 0, 0, 0, 0, 1)
K = len(FRACTIONS)
PLAIN = (0, 1, 2, 3, 4, 5)  # the fits compared in the run without l1 weights
FAMILY = 6                  # the fit compared in the run under the l1 weights

# the largest relative gap (relgap: every field and history entry, none excluded) between the restatement of each object's
# x-update and penalty_restated.run over SHAPES x MODES x the seven fits x nodualerror 0 | 1, as
# test_grouplasso_multi_host.test_restatement_matches_the_reference_and_measures_the_parity_gap printed it; the device's
# bound is 10x this (q37's margin: its summation order inside the products)
# dense 9.925e-12 (the 1.25*lambda_max fit on 600x257, per-fit S) and sparse 8.925e-10
MEASURED_GAP = dict(dense=1.0e-11, sparse=9.0e-10)
PARITY_BOUND = {kind: 10.0 * gap for kind, gap in MEASURED_GAP.items()}
assert max(PARITY_BOUND.values()) <= 1e-6  # never looser than the project's parity definition


def sizes_for(n):
    """contiguous groups that sum to n: a group of one, a group that ends short of 32, a group of 40 that crosses row 32
    (and is longer than a row block), then groups of 9 -- which cross every later multiple of 32 -- and the remainder"""
    head = [1, 20, 40]
    rest = n - sum(head)
    assert rest >= 1
    return head + [9] * (rest // 9) + ([rest % 9] if rest % 9 else [])


def group_lambda_max(A, s, sizes, gw):
    g = A.T @ s
    off = np.concatenate([[0], np.cumsum(sizes)])
    return max(float(np.linalg.norm(g[off[j]:off[j + 1]])) / gw[j] for j in range(len(sizes)) if gw[j] > 0)


_CACHE = {}
_REFS = {}


def case(ap, kind, shape, mode):
    """the base module's case of (shape, mode) plus sizes, gw (sqrt(p_g)), lams (the group strengths) and l1 (K values)"""
    key = (kind, tuple(shape), mode)
    if key not in _CACHE:
        c = dict((LM if kind == "dense" else SL).case(ap, shape, mode))
        n = c["A"].shape[1]
        sizes = sizes_for(n)
        gw = np.sqrt(np.asarray(sizes, dtype=np.float64))
        glmax = np.array([group_lambda_max(c["A"], SL.response(c, k), sizes, gw) for k in range(K)])
        c.update(sizes=np.asarray(sizes, dtype=np.int64), gw=gw, glmax=glmax, lams=np.asarray(FRACTIONS) * glmax,
                 l1=np.asarray(L1_FRACTIONS) * c["lmax"])
        _CACHE[key] = c
    return _CACHE[key]


def penalty_of(c, k, weighted):
    return PR.Penalty(l1weights=c["w"] if weighted else None, ridge=RIDGE[k], nonnegative=NONNEG[k],
                      sizes=c["sizes"], groupweights=c["gw"], l1=float(c["l1"][k]))


def fit_options(c, k, nodualerror, **more):
    return dict(SL.fit_options(c, k, nodualerror, **more), rho=RHO)


def reference_fit(ap, kind, shape, mode, k, nodualerror):
    """penalty_restated.run of fit k of (kind, shape, mode), computed once"""
    key = (kind, tuple(shape), mode, k, nodualerror)
    if key not in _REFS:
        c = case(ap, kind, shape, mode)
        _REFS[key] = PR.run(c["A"], SL.response(c, k), float(c["lams"][k]), penalty_of(c, k, k == FAMILY),
                            fit_options(c, k, nodualerror))
    return _REFS[key]


def restated_fit(kind, c, k, nodualerror):
    """one fit with the x-update of the object of `kind`"""
    A, s, lam = c["A"], SL.response(c, k), float(c["lams"][k])
    pen = penalty_of(c, k, k == FAMILY)
    n = A.shape[1]
    xsolve = LM.InverseSolve(A, A.T @ s, RHO) if kind == "dense" else SL.CgShift(A, A.T @ s, 1e-12, 200)
    o = fit_options(c, k, nodualerror)
    o["obj"] = lambda x, z: PR.objective(A, s, lam, pen, x, z)
    o.update(A=1, At=1, m=n, nA=n, nB=n, B=-1, c=0, parallel="none")
    return admm_ref.admm(xsolve, lambda x, _z, u, r: PR.prox(x + u, pen, pen.l1 / r, lam / r, r), o)
