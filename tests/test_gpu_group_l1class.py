"""The group and sparse-group penalty on the two sparse-linear-classifier objects on the device: the K
lock-step runs of groupclassifier_multi against the restated run (group_l1class_restated) per iteration and free-running,
on a dense and on a sparse D; two chunks (bits), groups set and taken back (bits), groups of one against the l1 form,
lambda >= lambda_max, folds and groups in both orders, the cross-validation, the path, the tester, the C ABI and the
setters' refusals.

Bounds.  Dense D: the project's 1e-6 (test_gpu_l1class.BOUND).  Sparse D: 10x the largest relative gap between the CG
restatement and the Cholesky one over these exact runs, measured on the CPU and recorded in group_l1class_restated
(test_group_l1class_host measures it again).  The l1 weights are shared by an object: every problem runs in two objects,
fits 0 .. 5 without them and the sparse-group fit with them."""
import ctypes as C

import numpy as np
import pytest

import group_l1class_restated as R
import sparse_l1class_cv_restated as CVR
from test_gpu_sparse_l1class import _compare_fit
from test_group_l1class_host import fold_masks

pytestmark = pytest.mark.gpu

KEYS = ("xopt", "zopt", "uopt", "pnorm", "perr", "dnorm", "derr", "objevals")
SMALL_D, SMALL_S = R.DENSE_SHAPES[0], R.SPARSE_SHAPES[0]


def _bound(c):
    return R.DENSE_BOUND if c["kind"] == "dense" else R.PARITY_BOUND


def _device(gpu, c, cols, loop, nodualerror, starts=True, **more):
    o, lams = R.device_options(c, cols, loop, nodualerror, starts, **more)
    return gpu.groupclassifier_multi(c["D"], c["ell"], lams, c["sizes"], o)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _same(a, i, b, j, steps=None):
    for key in KEYS:
        if key in a or key in b:
            rows = steps if key in KEYS[3:] else None
            assert _bits(a[key][:rows, i], b[key][:rows, j]), key


# ------------------------------------------------------------------------------------------ 1. parity per iteration
@pytest.mark.parametrize("nodualerror", (0, 1))
@pytest.mark.parametrize("shape", R.DENSE_SHAPES + R.SPARSE_SHAPES)
def test_every_iteration_matches_the_restated_run(gpu, shape, nodualerror):
    c = R.case(gpu, shape)
    dual = not nodualerror
    m, n = c["A"].shape
    got = _device(gpu, c, R.PLAIN, R.PARITY_LOOP, nodualerror)
    assert np.array_equal(got["groups"], c["sizes"]) and ("dnorm" in got) == dual
    assert got["zopt"].shape == (m + n, len(R.PLAIN)) and got["pnorm"].shape == (R.PARITY_LOOP["maxiters"], len(R.PLAIN))
    for k in R.PLAIN:
        ref = R.reference_fit(gpu, shape, k, R.PARITY_LOOP, nodualerror)
        _compare_fit(got, k, ref, dual, _bound(c))
        assert np.array_equal(R.groups_alive(got["zopt"][m:, k], c["sizes"]),
                              R.groups_alive(np.asarray(ref["zopt"])[m:], c["sizes"]))  # the support, exactly
    fam = _device(gpu, c, [R.FAMILY], R.PARITY_LOOP, nodualerror)
    ref = R.reference_fit(gpu, shape, R.FAMILY, R.PARITY_LOOP, nodualerror)
    _compare_fit(fam, 0, ref, dual, _bound(c))
    assert np.all(fam["zopt"][m:, 0] >= 0.0)
    assert np.array_equal(fam["zopt"][m:, 0] != 0, np.asarray(ref["zopt"])[m:] != 0)


@pytest.mark.parametrize("shape", (SMALL_D, SMALL_S))
def test_free_running_fits_take_the_steps_of_the_restated_runs(gpu, shape):
    c = R.case(gpu, shape)
    refs = [R.reference_fit(gpu, shape, k, None, 1, free=True) for k in range(R.K)]
    print("reference steps", [r["steps"] for r in refs])
    got = _device(gpu, c, R.PLAIN, dict(objevals=1), 1, starts=False)
    for k in R.PLAIN:
        _compare_fit(got, k, refs[k], False, _bound(c))
    fam = _device(gpu, c, [R.FAMILY], dict(objevals=1), 1, starts=False)
    _compare_fit(fam, 0, refs[R.FAMILY], False, _bound(c))


def test_wide_a_workgroup_walks_several_row_blocks(gpu):
    """n = 8300 under groups of 7 and one group of 300: the plan's budget doubles to 64 rows"""
    c = R.case(gpu, R.WIDE)
    got = _device(gpu, c, R.WIDE_FITS, R.WIDE_LOOP, 0)
    for i, k in enumerate(R.WIDE_FITS):
        _compare_fit(got, i, R.reference_fit(gpu, R.WIDE, k, R.WIDE_LOOP, 0), True, R.PARITY_BOUND)


# ------------------------------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("shape", (SMALL_D, SMALL_S))
def test_two_chunks_fits_alone_and_a_rerun_give_the_same_bits(gpu, shape):
    c = R.case(gpu, shape)
    cols = [k % len(R.PLAIN) for k in range(11)] + [0]
    loop = dict(objevals=1, maxiters=60)  # the free-running references stop at 21 .. 54 steps (test_group_l1class_host)
    got = _device(gpu, c, cols, loop, 1, starts=False)
    again = _device(gpu, c, cols, loop, 1, starts=False)
    steps = [int(s) for s in got["steps"]]
    print("steps", steps)
    assert got["xopt"].shape[1] == 12 and min(steps) < max(steps)  # a fit stops and stays frozen while others run on
    assert "dnorm" not in got  # (nodualerror = 1: the references' stop rule)
    for key in KEYS:
        if key in got:
            assert np.array_equal(got[key], again[key], equal_nan=True), key
    for twin in (6, 11):  # fit 0 again in the first chunk and in the second
        _same(got, 0, got, twin)
    for k in (0, 3, 4):
        one = _device(gpu, c, [k], loop, 1, starts=False)
        s = int(one["steps"][0])
        assert s == steps[k]
        _same(one, 0, got, k, s)
        assert np.isnan(got["pnorm"][s:, k]).all()


@pytest.mark.parametrize("shape", (SMALL_D, SMALL_S))
def test_groups_taken_back_restore_the_ungrouped_bits(gpu, shape):
    """set_groups(None) behind set_groups: l1classifier_multi's results; and groups may change between runs"""
    c = R.case(gpu, shape)
    fits = [c["fits"][k] for k in R.PLAIN]
    lams = [0.3 * f.lam for f in fits]
    losses = [f.loss for f in fits]
    cls = gpu.L1Classifier if c["kind"] == "dense" else gpu.SparseL1Classifier
    z0, u0 = np.asfortranarray(c["z0"][:, :6]), np.asfortranarray(c["u0"][:, :6])
    go = lambda o: o.results(o.run(objevals=1, maxiters=15, domaxiters=1, z0=z0, u0=u0))
    plain = gpu.l1classifier_multi(c["D"], c["ell"], lams, dict(lossfunction=losses, objevals=1, maxiters=15, domaxiters=1,
                                                                 z0=z0, u0=u0))
    obj = cls(c["D"], c["ell"], lams, losses)
    try:
        obj.set_groups(c["sizes"], c["gw"])
        grouped = go(obj)
        obj.set_groups([c["A"].shape[1]])
        one_group = go(obj)
        obj.set_groups(c["sizes"], c["gw"])
        grouped2 = go(obj)
        obj.set_groups(None)
        back = go(obj)
    finally:
        obj.close()
    for key in KEYS:
        assert _bits(back[key], plain[key]), key
        assert _bits(grouped[key], grouped2[key]), key
    assert not _bits(grouped["zopt"], plain["zopt"]) and not _bits(grouped["zopt"], one_group["zopt"])


@pytest.mark.parametrize("shape", (SMALL_D, SMALL_S))
def test_groups_of_one_agree_with_the_l1_form(gpu, shape):
    """sizes all 1, l1 = 0, groupweights w: the same minimiser and iteration as l1weights = w in another arithmetic form"""
    c = R.case(gpu, shape)
    n = c["A"].shape[1]
    w = c["lw"]
    lams = [0.1 * R.LR.lambda_max(c["A"], c["ell"], R.LR.Fit(loss=loss, l1weights=w)) for loss in ("logistic", "sqhinge")]
    o = dict(R.PARITY_LOOP, lossfunction=["logistic", "sqhinge"], z0=np.asfortranarray(c["z0"][:, :2]),
             u0=np.asfortranarray(c["u0"][:, :2]))
    if c["kind"] == "sparse":
        o["cg_tol"] = R.CG_TOL
    a = gpu.groupclassifier_multi(c["D"], c["ell"], lams, np.ones(n), dict(o, groupweights=w))
    b = gpu.l1classifier_multi(c["D"], c["ell"], lams, dict(o, l1weights=w))
    assert np.array_equal(a["steps"], b["steps"])
    for key in KEYS:
        scale = float(np.max(np.abs(b[key])))
        assert float(np.max(np.abs(a[key] - b[key]))) <= _bound(c) * scale, key


@pytest.mark.parametrize("shape", (SMALL_D, SMALL_S))
def test_at_lambda_max_with_every_group_penalised_z2_is_zero(gpu, shape):
    c = R.case(gpu, shape)
    m, n = c["A"].shape
    gw = np.sqrt(c["sizes"].astype(np.float64))
    lmax = gpu.groupclassifier_lambda_max(c["D"], c["ell"], c["sizes"], dict(groupweights=gw))
    res = gpu.groupclassifier_multi(c["D"], c["ell"], [lmax, 1.5 * lmax], c["sizes"], dict(groupweights=gw, objevals=1))
    assert np.all(res["zopt"][m:] == 0.0) and np.all(res["steps"] < 1000)


# ------------------------------------------------------------------------------------------ 3. folds
@pytest.mark.parametrize("order", ("folds_first", "groups_first"))
def test_folds_and_groups_in_both_orders_equal_the_masked_weight_run(gpu, order):
    c = R.case(gpu, SMALL_S)
    fold, held, masks = fold_masks(gpu, SMALL_S)
    fits = [c["fits"][k] for k in R.PLAIN]
    obj = gpu.SparseL1Classifier(c["D"], c["ell"], [f.lam for f in fits], [f.loss for f in fits])
    try:
        if order == "folds_first":
            obj.set_folds(fold, held[:6])
            obj.set_groups(c["sizes"], c["gw"])
        else:
            obj.set_groups(c["sizes"], c["gw"])
            obj.set_folds(fold, held[:6])
        got = obj.results(obj.run(cg_tol=R.CG_TOL, z0=np.asfortranarray(c["z0"][:, :6]), u0=np.asfortranarray(c["u0"][:, :6]),
                                  **R.PARITY_LOOP))
        loss, err, wt = obj.heldout()
    finally:
        obj.close()
    for k in R.PLAIN:
        ref = R.reference_fit(gpu, SMALL_S, k, R.PARITY_LOOP, 0, weights=masks[k])
        _compare_fit(got, k, ref, True, R.PARITY_BOUND)
        assert wt[k] == float(np.sum(fold == held[k]))


def test_groupclassifier_cv_agrees_with_the_restated_sums(gpu):
    cv = R.cv_case(gpu)
    F, L = R.CV_FOLDS, R.CV_NLAMBDA
    res = gpu.groupclassifier_cv(cv["D"], cv["ell"], cv["sizes"], cv["lams"],
                                 dict(R.CV_LOOP, groupweights=cv["gw"], nfolds=F, foldid=cv["foldid"], cg_tol=R.CG_TOL))
    sums = np.zeros((3, F, L))
    for f in range(F):
        for l in range(L):
            ref = R.cv_fit(gpu, f, l)
            assert int(res["fold_steps"][f, l]) == ref["steps"]
            sums[:, f, l] = CVR.heldout_sums(cv["A"], cv["ell"], np.ones(cv["ell"].size), "logistic", cv["foldid"], f,
                                             np.asarray(ref["zopt"]))[:3]
    assert np.array_equal(res["heldout_weight"], sums[2]) and np.allclose(res["fold_lams"], cv["fold_lams"], rtol=1e-15)
    tol = R.PARITY_BOUND * R.LOSS_CONDITION  # q47's rule: the parity bound through the loss sums' condition
    gap = float(np.max(np.abs(res["heldout_loss"] - sums[0]) / np.abs(sums[0])))
    print(f"held-out loss: relative gap {gap:.3e} (bound {tol:.3e})")
    assert gap <= tol
    want = gpu.solvers.cv_summary(sums[0], sums[2], cv["lams"])
    assert np.max(np.abs(res["cvm"] - want["cvm"]) / np.abs(want["cvm"])) <= tol
    assert res["index_min"] == want["index_min"] and res["lam_min"] == want["lam_min"]
    assert res["index_1se"] == want["index_1se"] and res["lam_1se"] == want["lam_1se"]
    m = cv["ell"].size
    for l in range(L):
        ref = R.cv_fit(gpu, F, l)
        assert int(res["steps"][l]) == ref["steps"]
        assert np.array_equal(R.groups_alive(res["zopt"][m:, l], cv["sizes"]),
                              R.groups_alive(np.asarray(ref["zopt"])[m:], cv["sizes"]))
    assert np.array_equal(res["groups"], cv["sizes"]) and res["df_groups"].shape == (L,)


# ------------------------------------------------------------------------------------------ 4. path, tester, C ABI
@pytest.mark.parametrize("shape", (SMALL_D, SMALL_S))
def test_path_starts_at_lambda_max_with_no_group(gpu, shape):
    c = R.case(gpu, shape)
    gw = np.sqrt(c["sizes"].astype(np.float64))
    res = gpu.groupclassifier_path(c["D"], c["ell"], c["sizes"], None, dict(groupweights=gw))
    lmax = R.lambda_max(c["A"], c["ell"], R.Fit(c["sizes"], gw))
    assert res["lams"].shape == (10,) and np.all(np.diff(res["lams"]) < 0) and abs(res["lams"][0] - lmax) <= 1e-14 * lmax
    assert res["df_groups"][0] == 0 and res["df"][0] == 0 and res["df_groups"][-1] > 0
    assert np.all(res["df_groups"] <= len(c["sizes"])) and np.array_equal(res["groups"], c["sizes"])
    one = gpu.groupclassifier(c["D"], c["ell"], float(res["lams"][4]), c["sizes"], dict(groupweights=gw))
    assert one["xopt"].shape == (c["A"].shape[1],) and isinstance(one["steps"], int) and one["steps"] == int(res["steps"][4])


@pytest.mark.parametrize("sparse", (True, False))
def test_the_tester(gpu, sparse):
    _, test = gpu.testers.groupclassifiertest(sparse=sparse)
    print({k: test[k] for k in ("used_found", "unused_found", "accuracy", "steps")})
    assert test["failed"] == 0


def _raw_groups(L, fn, h, sizes, gw=None, l1=None):
    sz = None if sizes is None else np.ascontiguousarray(sizes, dtype=np.int64)
    keep = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (gw, l1)]
    return fn(h, 0 if sz is None else sz.size, None if sz is None else sz.ctypes.data_as(C.POINTER(C.c_int64)),
              None if keep[0] is None else L.as_dp(keep[0]), None if keep[1] is None else L.as_dp(keep[1]))


@pytest.mark.parametrize("shape", (SMALL_D, SMALL_S))
def test_bare_c_abi_sequence_and_refusals_that_change_nothing(gpu, shape):
    """create / set_groups / run / run with another rho / destroy through the bare entry points of the owner's handle; a
    refused set_groups leaves the object as it was: the following run's bits say so"""
    L = gpu._lib
    lib = L.load()
    c = R.case(gpu, shape)
    dense = c["kind"] == "dense"
    fn = lib.admm_group_l1class_set_groups if dense else lib.admm_sparse_l1class_set_groups
    cls = gpu.L1Classifier if dense else gpu.SparseL1Classifier
    fits = [c["fits"][k] for k in (1, 4, 5)]
    n = c["A"].shape[1]
    z0, u0 = np.asfortranarray(c["z0"][:, :3]), np.asfortranarray(c["u0"][:, :3])
    obj = cls(c["D"], c["ell"], [f.lam for f in fits], [f.loss for f in fits])
    go = lambda rho: obj.results(obj.run(objevals=1, maxiters=12, domaxiters=1, rho=rho, z0=z0, u0=u0))
    try:
        assert _raw_groups(L, fn, obj._h, c["sizes"], c["gw"], [0.0, 0.01, 0.0]) == 0
        first, second = go(1.0), go(2.5)
        assert not _bits(first["zopt"], second["zopt"])
        bad = c["sizes"].copy()
        bad[1] = 0
        for sizes, gw, l1, code, part in (
                (bad, None, None, L.E_INVALID, "group 1 has a size below 1"),
                (c["sizes"][:-1], None, None, L.E_INVALID, f"not to n = {n}"),
                (c["sizes"], np.where(np.arange(len(c["sizes"])) == 2, -1.0, 1.0), None, L.E_INVALID, "weight 2 is negative"),
                (c["sizes"], c["gw"], [0.0, np.nan, 0.0], L.E_INVALID, "fit 1: l1 is negative or not finite")):
            assert _raw_groups(L, fn, obj._h, sizes, gw, l1) == code
            assert part in lib.admm_last_error().decode()
        assert fn(None, 0, None, None, None) == L.E_INVALID
        with pytest.raises(ValueError, match="every size must be an integer"):
            obj.set_groups([1.5, n - 1.5])
        kept = go(2.5)
        for key in KEYS:
            assert _bits(kept[key], second[key]), key
        assert _raw_groups(L, fn, obj._h, None) == 0  # G = 0: the ungrouped prox again
        plain = go(2.5)
    finally:
        obj.close()
    ref = gpu.l1classifier_multi(c["D"], c["ell"], [f.lam for f in fits],
                                 dict(lossfunction=[f.loss for f in fits], objevals=1, maxiters=12, domaxiters=1, rho=2.5,
                                      z0=z0, u0=u0))
    for key in KEYS:
        assert _bits(plain[key], ref[key]), key


def test_kernel_time_times_the_grouped_element_kernel(gpu):
    c = R.case(gpu, SMALL_S)
    obj = gpu.SparseL1Classifier(c["D"], c["ell"], [c["fits"][1].lam], ["logistic"])
    try:
        obj.set_groups(c["sizes"], c["gw"])
        t = obj.kernel_time(reps=3)
    finally:
        obj.close()
    assert t["elem_us"] > 0.0 and t["row_us"] > 0.0
