"""The group and sparse-group penalty on the sparse linear classifiers, no device: the restatement
(group_l1class_restated) against the group lasso's optimality conditions, its CG form against its Cholesky form over every
run the sparse GPU test compares (the measured gap the device bound is derived from), the conditions the GPU tests rely
on -- asserted on the reference alone --, the plan of the grouped element kernel for the group sizes of the GPU tests,
groupclassifier_lambda_max, and every refusal that needs no device."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import group_l1class_restated as R
import sparse_l1class_cv_restated as CVR
from test_grouplasso_multi_host import _plan


# ------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("loss, fraction", (("logistic", 0.15), ("sqhinge", 0.5)))
def test_a_converged_restated_fit_meets_the_group_kkt_conditions(ap, loss, fraction):
    c = R.case(ap, R.DENSE_SHAPES[0])
    f = R.Fit(c["sizes"], c["gw"], loss=loss)
    f.lam = fraction * R.lambda_max(c["A"], c["ell"], f)
    res = R.run(c["A"], c["ell"], f, dict(abstol=1e-13, reltol=1e-11, maxiters=20000))
    m = c["A"].shape[0]
    z2 = np.asarray(res["zopt"])[m:]
    alive = R.groups_alive(z2, c["sizes"])
    v = R.kkt(c["A"], c["ell"], f, z2)
    print(f"{loss}: steps {res['steps']}, groups alive {int(alive.sum())} of {alive.size}, kkt {v:.3e}, lam {f.lam:.3e}")
    assert res["steps"] < 20000 and alive[0] and 1 < alive.sum() < alive.size  # a model between the two trivial ones
    assert v <= 1e-7 * f.lam


# ------------------------------------------------------------------------------------------ 2. the measured gap
def _gap(ap, shape, k, loop, nd, free=False, weights=None):
    a = R.reference_fit(ap, shape, k, loop, nd, free, "cg", weights)
    b = R.reference_fit(ap, shape, k, loop, nd, free, "chol", weights)
    assert a["steps"] == b["steps"], (shape, k, nd, a["steps"], b["steps"])
    return R.relgap(a, b)


def fold_masks(ap, shape):
    """the folds test's fold ids, held-out folds of the seven fits and masked weight vectors"""
    m = R.case(ap, shape)["ell"].size
    fold = ap.solvers.cv_folds(m, 3, 1)
    held = np.array([0, 1, 2, -1, 0, 1, 2])
    return fold, held, [(fold != h).astype(np.float64) for h in held]


def test_cg_restatement_against_cholesky_measures_the_gap(ap):
    worst = 0.0
    for shape in R.SPARSE_SHAPES:
        for nd in (0, 1):
            for k in range(R.K):
                worst = max(worst, _gap(ap, shape, k, R.PARITY_LOOP, nd))
        print(f"{shape} forced: {worst:.3e}")
    for k in range(R.K):
        worst = max(worst, _gap(ap, R.SPARSE_SHAPES[0], k, None, 1, free=True))
    print(f"free-running: {worst:.3e}")
    for k in R.WIDE_FITS:
        worst = max(worst, _gap(ap, R.WIDE, k, R.WIDE_LOOP, 0))
    print(f"WIDE: {worst:.3e}")
    _, _, masks = fold_masks(ap, R.SPARSE_SHAPES[0])
    for k in R.PLAIN:
        worst = max(worst, _gap(ap, R.SPARSE_SHAPES[0], k, R.PARITY_LOOP, 0, weights=masks[k]))
    print(f"folds: {worst:.3e}")
    for f in range(R.CV_FOLDS + 1):
        for l in range(R.CV_NLAMBDA):
            a, b = R.cv_fit(ap, f, l, "cg"), R.cv_fit(ap, f, l, "chol")
            assert a["steps"] == b["steps"]
            worst = max(worst, R.relgap(a, b))
    print(f"largest gap {worst:.3e} (recorded {R.MEASURED_GAP:g})")
    assert worst <= R.MEASURED_GAP
    assert R.PARITY_BOUND == 10.0 * R.MEASURED_GAP and R.PARITY_BOUND <= 1e-6 and R.DENSE_BOUND == 1e-6


# ------------------------------------------------------------------------------------------ 4. the conditions
def _stop_margins(ref, dual):
    """(at the stop, one step earlier): the relative distance of the residuals from their tolerances"""
    s = ref["steps"]
    out = []
    for i in (s - 1, s - 2):
        if i < 0:
            continue
        d = [abs(ref["pnorm"][i] - ref["perr"][i]) / ref["perr"][i]]
        if dual:
            d.append(abs(ref["dnorm"][i] - ref["derr"][i]) / ref["derr"][i])
        out.append(min(d))
    return min(out)


@pytest.mark.parametrize("shape", (R.DENSE_SHAPES[0], R.SPARSE_SHAPES[0]))
def test_the_conditions_hold_on_the_reference(ap, shape):
    c = R.case(ap, shape)
    bound = R.DENSE_BOUND if c["kind"] == "dense" else R.PARITY_BOUND
    refs = [R.reference_fit(ap, shape, k, None, 1, free=True) for k in range(R.K)]
    steps = [r["steps"] for r in refs]
    print(shape, "reference steps", steps)
    assert len(set(steps)) >= R.FREE_DISTINCT and max(steps) < 1000
    for k, r in enumerate(refs):
        assert _stop_margins(r, False) > 1e-6, (k, _stop_margins(r, False))
        margin = R.threshold_margin(c, k, r, 1.0)
        print(f"fit {k}: steps {r['steps']}, threshold margin {margin:.3e}")
        assert margin > 1e3 * bound, (k, margin)  # no group within the bound's reach of its threshold


@pytest.mark.parametrize("shape", R.DENSE_SHAPES + R.SPARSE_SHAPES)
def test_forced_runs_keep_every_group_away_from_its_threshold(ap, shape):
    c = R.case(ap, shape)
    bound = R.DENSE_BOUND if c["kind"] == "dense" else R.PARITY_BOUND
    for k in range(R.K):
        r = R.reference_fit(ap, shape, k, R.PARITY_LOOP, 0)
        assert R.threshold_margin(c, k, r, R.PARITY_LOOP["rho"]) > 1e2 * bound, k
    m = c["A"].shape[0]
    assert np.all(np.asarray(R.reference_fit(ap, shape, R.FAMILY, R.PARITY_LOOP, 0)["zopt"])[m:] >= 0.0)


def test_cv_loss_condition(ap):
    """sparse_l1class_cv_restated.LOSS_CONDITION's measure on this cross-validation's fold fits"""
    cv = R.cv_case(ap)
    worst = 0.0
    for f in range(R.CV_FOLDS):
        for l in range(R.CV_NLAMBDA):
            cc = dict(A=cv["A"], ell=cv["ell"], fold=cv["foldid"], held=np.array([f]),
                      fits=[R.LR.Fit(loss="logistic")])
            worst = max(worst, CVR.loss_condition(cc, 0, np.asarray(R.cv_fit(ap, f, l)["zopt"])))
    print(f"loss condition {worst:.4g} (recorded {R.LOSS_CONDITION:g})")
    assert 0.0 < worst <= R.LOSS_CONDITION


# ------------------------------------------------------------------------------------------ 5. the plan
@pytest.mark.parametrize("n", (70, 130, 65, 200))
def test_plan_of_the_small_problems_is_one_workgroup_per_budget(ap, n):
    sizes = R.sizes_for(n)
    rc, first, budget = _plan(ap, n, sizes)
    off = R.offsets(sizes)
    assert rc == 0 and budget == 32 and first[0] == 0 and first[-1] == n and set(first) <= set(off)
    assert list(first[:3]) == [0, 21, 61]  # 1 + 20 fit one row block; the group of 40 stands alone


def test_plan_of_the_wide_problem_doubles_the_budget(ap):
    rc, first, budget = _plan(ap, R.WIDE[1], R.WIDE_SIZES)
    off = R.offsets(R.WIDE_SIZES)
    assert rc == 0 and budget == 64 and len(first) - 1 <= 256 and set(first) <= set(off)
    rows = np.diff(first)
    assert rows.max() == 300 and np.sum(rows > 32) > 100  # a workgroup walks several row blocks
    assert np.all((rows <= budget) | (rows == 300))


# ------------------------------------------------------------------------------------------ 6. lambda_max
@pytest.mark.parametrize("shape", (R.DENSE_SHAPES[0], R.SPARSE_SHAPES[1]))
def test_lambda_max_equals_the_restated_formula(ap, shape):
    c = R.case(ap, shape)
    for loss in ("logistic", "hinge", "sqhinge"):
        w = np.linspace(0.5, 2.0, c["ell"].size)
        f = R.Fit(c["sizes"], c["gw"], loss=loss, weights=w, classcost=(2.0, 0.5), C=3.0)
        got = ap.groupclassifier_lambda_max(c["D"], c["ell"], c["sizes"],
                                            dict(groupweights=c["gw"], lossfunction=loss, weights=w, classcost=(2.0, 0.5), C=3.0))
        ref = R.lambda_max(c["A"], c["ell"], f)
        assert abs(got - ref) <= 1e-14 * ref, (loss, got, ref)
    ones = ap.groupclassifier_lambda_max(c["D"], c["ell"], np.ones(c["A"].shape[1]))
    assert abs(ones - ap.l1classifier_lambda_max(c["D"], c["ell"])) <= 1e-14 * ones  # groups of one: the l1 formula


# ------------------------------------------------------------------------------------------ 7. refusals
def _data():
    p = R.LR.problem((40, 12), K=2)
    return p["D"], p["ELL"]


@pytest.mark.parametrize("call, message", (
    (lambda ap, D, E: ap.groupclassifier(D, E[:, 0], 0.1, [6, 5]), "sum to 11, not to the 12 columns"),
    (lambda ap, D, E: ap.groupclassifier(D, E[:, 0], 0.1, [6, 5.5, 0.5]), "every size must be an integer"),
    (lambda ap, D, E: ap.groupclassifier(D, E[:, 0], 0.1, [12, 0]), "every size must be >= 1"),
    (lambda ap, D, E: ap.groupclassifier(D, E[:, 0], 0.1, []), "at least one group size"),
    (lambda ap, D, E: ap.groupclassifier(D, E[:, 0], 0.1, [6, 6], dict(groupweights=[1.0])), "groupweights has 1 entries"),
    (lambda ap, D, E: ap.groupclassifier(D, E[:, 0], 0.1, [6, 6], dict(groupweights=[1.0, -1.0])), "finite and >= 0"),
    (lambda ap, D, E: ap.groupclassifier(D, E[:, 0], 0.1, [6, 6], dict(l1=-1.0)), "fit 0"),
    (lambda ap, D, E: ap.groupclassifier(D, E[:, 0], 0.1, [6, 6], dict(l1=[0.1, 0.2])), "options.l1"),
    (lambda ap, D, E: ap.groupclassifier_multi(D, E, [0.1, 0.2], [6, 6], dict(l1=[0.1, 0.2, 0.3])), "l1 has 3 entries for 2 fits"),
    (lambda ap, D, E: ap.groupclassifier_multi(D, E, [0.1, -0.2], [6, 6]), "fit 1: lambda"),
    (lambda ap, D, E: ap.groupclassifier_multi(D, E, [0.1, 0.2], [6, 6], dict(lossfunction="01")), "0-1 loss is not convex"),
    (lambda ap, D, E: ap.groupclassifier_multi(D, E, [0.1, 0.2], [6, 6], dict(fast=1)), "options.fast is not available in groupclassifier_multi"),
    (lambda ap, D, E: ap.groupclassifier_multi(D, E, [0.1, 0.2], [6, 6], dict(foldid=np.zeros(40), heldout=[0, 0])),
     "options.foldid is not available in groupclassifier_multi"),
    (lambda ap, D, E: ap.groupclassifier_multi(sp.csc_matrix(D), E, [0.1, 0.2], [6, 6], dict(obsweights=np.ones(40))),
     "options.obsweights is not available in groupclassifier_multi"),
    (lambda ap, D, E: ap.groupclassifier_multi(sp.csc_matrix(D), E, [0.1, 0.2], [6, 6], dict(foldid=np.zeros(40))),
     "options.foldid needs options.heldout"),
    (lambda ap, D, E: ap.groupclassifier_multi(sp.csc_matrix(D), E, [0.1, 0.2], [6, 6], dict(xsolve="inverse")), "matrix-free"),
    (lambda ap, D, E: ap.groupclassifier_path(D, E[:, 0], [6, 6], None, dict(l1=0.1)), "lambda_max has no closed form: give lams"),
    (lambda ap, D, E: ap.groupclassifier_path(D, E[:, 0], [6, 6], 5, dict(l1=[0.0, 0.1, 0, 0, 0])), "give lams"),
    (lambda ap, D, E: ap.groupclassifier_path(D, E[:, 0], [6, 6], None, dict(nlambda=0)), "options.nlambda"),
    (lambda ap, D, E: ap.groupclassifier_cv(D, E[:, 0], [6, 6]), "groupclassifier_cv runs on a scipy.sparse D"),
    (lambda ap, D, E: ap.groupclassifier_cv(sp.csc_matrix(D), E[:, 0], [6, 5]), "sum to 11"),
    (lambda ap, D, E: ap.groupclassifier_cv(sp.csc_matrix(D), E[:, 0], [6, 6], None, dict(l1=0.1)), "give lams"),
    (lambda ap, D, E: ap.groupclassifier_cv(sp.csc_matrix(D), E[:, 0], [6, 6], [0.1], dict(heldout=[0])),
     "groupclassifier_cv's own to set"),
    (lambda ap, D, E: ap.groupclassifier_cv(sp.csc_matrix(D), E[:, 0], [6, 6], [0.1], dict(nfolds=1)), "options.nfolds"),
    (lambda ap, D, E: ap.groupclassifier_lambda_max(D, E[:, 0], [6, 5]), "sum to 11"),
    (lambda ap, D, E: ap.groupclassifier_lambda_max(D, E[:-1, 0], [6, 6]), "rows in argument D"),
))
def test_refusals_that_need_no_device(ap, call, message):
    D, E = _data()
    with pytest.raises(ValueError, match=message):
        call(ap, D, E)


def test_symbols_and_the_one_setter(ap):
    L = ap._lib
    for name in ("admm_group_l1class_set_groups", "admm_sparse_l1class_set_groups"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(L.load(), name)
    assert ap.L1Classifier.set_groups is ap.SparseL1Classifier.set_groups is ap.LassoMulti.set_groups
    hdr = open(ap._lib.HEADER).read() if hasattr(ap._lib, "HEADER") else None
    assert hdr is None or "admm_sparse_l1class_set_groups" in hdr
    for name in ("groupclassifier", "groupclassifier_multi", "groupclassifier_path", "groupclassifier_lambda_max",
                 "groupclassifier_cv"):
        assert callable(getattr(ap, name))
