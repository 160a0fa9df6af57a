"""The sparse l1 classifier under held-out folds on the device: twelve fits (three folds x three lambdas
and three full-data fits, two chunks) against the restatement of the full-row problem with zero-cost rows
(sparse_l1class_cv_restated) per iteration and free-running; the edge folds; the bitwise contracts; heldout(), the
setter's refusals and l1classifier_cv end to end.

Bounds.  Every field and history: 10x the largest gap between the CG restatement and the Cholesky restatement over these
exact runs, measured on the CPU by test_sparse_l1class_cv_host (MEASURED_GAP = 8.3e-12).  The held-out loss and cvm: that
bound times LOSS_CONDITION (185, measured there).  The held-out weight, the weighted errors, the support of z2 and the two
indices are compared exactly: test_the_two_conditions_hold asserts on the reference alone that they may be.  Free-running
parity runs under nodualerror = 1 only: under nodualerror = 0 the small-lambda runs cost the restatement 15 - 25 s each."""
import ctypes as C

import numpy as np
import pytest

import sparse_l1class_cv_restated as W
from sparse_cases import csc_of
from test_gpu_sparse_l1class import KEYS, _compare_fit
from test_gpu_sparse_lasso import _close
from test_sparse_l1class_host import raw_create

pytestmark = pytest.mark.gpu

BOUND = W.PARITY_BOUND
LOSS_BOUND = BOUND * W.LOSS_CONDITION


def _options(c, cols, loop, nodualerror, starts=True, folds=True, weights="case"):
    fits = [c["fits"][k] for k in cols]
    o = dict(loop, lossfunction=[f.loss for f in fits], nodualerror=nodualerror, cg_tol=W.CG_TOL)
    w = c["weights"] if isinstance(weights, str) else weights
    if w is not None:
        o["weights"] = w
    if c["classcost"] is not None:
        o["classcost"] = np.ascontiguousarray(c["classcost"][cols])
    if folds:
        o.update(foldid=c["fold"], heldout=c["held"][cols])
    if starts:
        o.update(z0=np.asfortranarray(c["z0"][:, cols]), u0=np.asfortranarray(c["u0"][:, cols]))
    return o


def _device(gpu, c, cols, loop, nodualerror, **kw):
    cols = list(cols)
    return gpu.l1classifier_multi(c["D"], c["ell"], [c["fits"][k].lam for k in cols], _options(c, cols, loop, nodualerror, **kw))


def _compare_heldout(got, i, c, k, ref):
    """column i of a result against the restated sums of fit k: the loss at its bound, errors, weight and the support of
    z2 exactly"""
    m = c["A"].shape[0]
    loss, err, wt, _ = W.fit_sums(c, k, np.asarray(ref["zopt"]))
    assert np.array_equal(got["zopt"][m:, i] != 0, np.asarray(ref["zopt"])[m:] != 0), k
    print(f"fit {k}: held-out loss {got['heldout_loss'][i]:.12e} / {loss:.12e}, errors {got['heldout_errors'][i]} / {err}, "
          f"weight {got['heldout_weight'][i]} / {wt}")
    assert got["heldout_weight"][i] == wt and got["heldout_errors"][i] == err, k
    assert abs(got["heldout_loss"][i] - loss) <= LOSS_BOUND * loss, (k, got["heldout_loss"][i], loss)
    if c["held"][k] < 0 or wt == 0.0:
        assert got["heldout_loss"][i] == 0.0 and err == 0.0 and wt == 0.0


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _same_fit(a, i, b, j, keys=KEYS):
    s = int(a["steps"][i])
    assert s == int(b["steps"][j])
    for key in keys:
        rows = s if key in KEYS[3:] else None
        assert _bits(a[key][:rows, i], b[key][:rows, j]), (key, i, j)
    assert a["objopt"][i] == b["objopt"][j] and a["cg_iters_total"][i] == b["cg_iters_total"][j]


# ------------------------------------------------------------------------------------------ 1. parity per iteration
@pytest.mark.parametrize("nodualerror", (0, 1))
@pytest.mark.parametrize("obj", W.OBJECTS)
@pytest.mark.parametrize("shape", W.SHAPES)
def test_every_iteration_matches_the_restated_run(gpu, shape, obj, nodualerror):
    c = W.case(gpu, shape, obj)
    got = _device(gpu, c, range(W.K), W.PARITY_LOOP, nodualerror)
    assert got["chunk"] == 10 and got["xopt"].shape[1] == W.K == 12  # two chunks: fit 9 shares one with the full-data fits
    for k in range(W.K):
        ref = W.restated_fit(gpu, shape, obj, k, W.PARITY_LOOP, nodualerror)
        _compare_fit(got, k, ref, not nodualerror, BOUND)
        if nodualerror:  # (the runs test_the_two_conditions_hold covers)
            _compare_heldout(got, k, c, k, ref)
    assert not got["cg_capped_updates"].any()
    assert np.all(got["heldout_weight"][W.F * W.L:] == 0.0) and np.all(got["heldout_weight"][:W.F * W.L] > 0.0)
    # the contract on a held-out row: z1 = fl(D x + u1), so u1 + (D x - z1) is 0 up to the one rounding of that sum
    m = c["A"].shape[0]
    for k in (0, 4, 8):
        rows = c["fold"] == c["held"][k]
        z1 = got["zopt"][:m, k][rows]
        assert rows.any() and np.all(np.abs(got["uopt"][:m, k][rows]) <= 2.0 ** -52 * np.max(np.abs(z1)))


# ---------------------------------------------------------------------------------------------- 2. free-running
@pytest.mark.parametrize("shape", W.SHAPES)
def test_free_running_fits_stop_where_the_restated_runs_stop(gpu, shape):
    c = W.case(gpu, shape, "logistic")
    refs = [W.restated_fit(gpu, shape, "logistic", k, None, 1, free=True) for k in range(W.K)]
    steps = [r["steps"] for r in refs]
    print("reference steps", steps)
    assert len(set(steps[:W.F * W.L])) >= W.FREE_DISTINCT  # on the reference alone
    got = _device(gpu, c, range(W.K), dict(objevals=1), 1, starts=False)
    for k in range(W.K):
        _compare_fit(got, k, refs[k], False, BOUND)
        _compare_heldout(got, k, c, k, refs[k])
    assert not got["cg_capped_updates"].any()


# ---------------------------------------------------------------------------------------------- 3. edge shapes
@pytest.mark.parametrize("shape", (W.SHAPES[0], W.EDGE_M))
def test_edge_folds(gpu, shape):
    """257 rows: fold 1 is exactly the second row block of kScgRows rows, fold 2 the dense row 3 and the empty row 5, fold
    3 has no rows; m = kScgRows + 1: the last row is a fold of its own"""
    c = W.edge_case(gpu, *W.edge_problem(shape))
    m = c["A"].shape[0]
    if m > 2 * W.ROWS:
        assert list(np.flatnonzero(c["fold"] == 1)) == list(range(W.ROWS, 2 * W.ROWS))
        assert list(np.flatnonzero(c["fold"] == 2)) == [3, 5] and not (c["fold"] == 3).any()
        assert np.count_nonzero(c["A"][3]) == c["A"].shape[1] - 1 and not c["A"][5].any()
    else:
        assert m == W.ROWS + 1 and list(np.flatnonzero(c["fold"] == 1)) == [W.ROWS]
    o = _options(c, list(range(W.K)), W.PARITY_LOOP, 0)
    got = gpu.l1classifier_multi(c["D"], c["ell"], [f.lam for f in c["fits"]], o)
    for k in range(W.K):
        ref = W.edge_fit(gpu, c, k)
        _compare_fit(got, k, ref, True, BOUND)
        _compare_heldout(got, k, c, k, ref)
    if m > 2 * W.ROWS:
        empty = np.flatnonzero(c["held"] == 3)
        assert empty.size == 2
        for key in ("heldout_loss", "heldout_errors", "heldout_weight"):
            assert np.all(got[key][empty] == 0.0), key
        # cv_summary skips a fold of zero weight
        F = W.EDGE_NFOLDS
        k_of = [int(np.flatnonzero(c["held"] == f)[0]) for f in range(F)]
        s = gpu.solvers.cv_summary(got["heldout_loss"][k_of].reshape(F, 1), got["heldout_weight"][k_of].reshape(F, 1), [1.0])
        live = [k for k in k_of if got["heldout_weight"][k] > 0]
        assert s["cvm"][0] == got["heldout_loss"][live].sum() / got["heldout_weight"][live].sum()
        assert np.isfinite(s["cvsd"][0])
        two = np.flatnonzero(c["held"] == 2)[0]  # the empty row: t = 0, an error of weight 1 and a loss of log 2
        assert got["heldout_weight"][two] == 2.0 and got["heldout_errors"][two] >= 1.0


# ---------------------------------------------------------------------------------------------- 4. bitwise contracts
def test_bitwise_contracts(gpu):
    c = W.case(gpu, W.SHAPES[0], "mixed")
    loop = dict(objevals=1, maxiters=40)
    cols = list(range(W.K))
    mixed = _device(gpu, c, cols, loop, 0)
    again = _device(gpu, c, cols, loop, 0)
    for key in KEYS + ("heldout_loss", "heldout_errors", "heldout_weight", "objopt"):
        assert np.array_equal(mixed[key], again[key], equal_nan=True), key  # a rerun
    steps = [int(s) for s in mixed["steps"]]
    print("steps", steps)
    # a held = -1 fit inside the mixed object equals the same fit in an object without folds
    plain = _device(gpu, c, cols, loop, 0, folds=False)
    assert "heldout_loss" not in plain
    for k in range(W.F * W.L, W.K):
        _same_fit(mixed, k, plain, k)
    # fold fit k equals the same fit in an object without folds whose weights are weights o [fold != held_k]
    for k in (1, 5, 9):
        w = c["weights"] * (c["fold"] != c["held"][k])
        one = _device(gpu, c, [k], loop, 0, folds=False, weights=w)
        _same_fit(one, 0, mixed, k)
        alone = _device(gpu, c, [k], loop, 0)  # a fold fit alone equals the same fit among 12
        _same_fit(alone, 0, mixed, k)
        for key in ("heldout_loss", "heldout_errors", "heldout_weight"):
            assert alone[key][0] == mixed[key][k], (key, k)


def test_set_folds_then_null_equals_the_object_that_never_had_folds(gpu):
    L = gpu._lib
    c = W.case(gpu, W.SHAPES[0], "mixed")
    cols = list(range(W.K))
    fits = c["fits"]
    z0, u0 = c["z0"], c["u0"]

    def make():
        o = gpu.SparseL1Classifier(c["D"], c["ell"], [f.lam for f in fits], [f.loss for f in fits])
        return o

    def go(obj):
        s = obj.run(objevals=1, maxiters=25, z0=z0, u0=u0)
        S = int(s["steps"].max())
        return [s["steps"], s["objopt"], s["cg_iters_total"]] + [obj.fetch(f, r) for f, r in (
            (L.L1C_F_XOPT, obj.n), (L.L1C_F_ZOPT, obj.mn), (L.L1C_F_UOPT, obj.mn), (L.L1C_F_PNORM, S), (L.L1C_F_DNORM, S),
            (L.L1C_F_OBJEVALS, S))]

    never, had = make(), make()
    try:
        never.set_cost(c["weights"], c["classcost"])
        want = go(never)
        with pytest.raises(RuntimeError, match="folds set"):  # refused without folds ...
            never.heldout()
        had.set_folds(c["fold"], c["held"])  # set_folds then set_cost: either order
        had.set_cost(c["weights"], c["classcost"])
        with pytest.raises(RuntimeError, match="folds set"):  # ... and before a run
            had.heldout()
        folded = go(had)
        loss, err, wt = had.heldout()
        assert np.all(wt[:W.F * W.L] > 0) and not np.array_equal(folded[3], want[3])
        other = make()
        try:
            other.set_cost(c["weights"], c["classcost"])  # set_cost then set_folds
            other.set_folds(c["fold"], c["held"])
            for a, b in zip(folded, go(other)):
                assert np.array_equal(a, b, equal_nan=True)
            assert all(np.array_equal(a, b) for a, b in zip((loss, err, wt), other.heldout()))
        finally:
            other.close()
        t = had.kernel_time(3, 1)  # the FOLD form, timed
        assert t["row_us"] > 0 and t["elem_us"] > 0
        had.set_folds(None, None)
        for a, b in zip(want, go(had)):
            assert a.size > 0 and np.array_equal(a, b, equal_nan=True)
        with pytest.raises(RuntimeError, match="folds set"):
            had.heldout()
    finally:
        never.close()
        had.close()


# ---------------------------------------------------------------------------------------------- 5. the setter's refusals
def test_setter_refusals_name_the_row_or_the_fit(gpu):
    L = gpu._lib
    lib = L.load()
    c = W.case(gpu, W.SHAPES[0], "logistic")
    rc, h = raw_create(L, csc_of(c["D"]), c["ell"].reshape(-1, 1), [0.1, 0.2, 0.3], xsolve=L.XSOLVE_CG)
    assert rc == L.OK and h.value, lib.admm_last_error()
    ip = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    fold = np.arange(257) % 3
    bad_row = fold.copy()
    bad_row[17] = 3
    neg_row = fold.copy()
    neg_row[200] = -1
    try:
        for nfolds, f, hd, needle in ((0, fold, [0, 1, 2], "nfolds must be at least 1"),
                                      (3, bad_row, [0, 1, 2], "row 17"), (3, neg_row, None, "row 200"),
                                      (3, fold, [0, 3, -1], "fit 1"), (3, fold, [0, 1, -2], "fit 2"),
                                      (3, None, [0, 1, 2], "heldout needs the fold ids")):
            keep = [None if a is None else np.ascontiguousarray(a, dtype=np.int32) for a in (f, hd)]
            rc = lib.admm_sparse_l1class_set_folds(h, nfolds, ip(keep[0]), ip(keep[1]))
            assert rc == L.E_INVALID and needle in lib.admm_last_error().decode(), (needle, lib.admm_last_error())
        one = np.zeros(3)
        assert lib.admm_sparse_l1class_heldout(h, L.as_dp(one), L.as_dp(one), L.as_dp(one)) == L.E_INVALID
        # a refused call changed nothing: the run is the run of an object without folds
        o = L.SparseL1ClassOptions()
        lib.admm_sparse_l1class_options_default(C.byref(o))
        o.maxiters, o.domaxiters = 5, 1
        L.check(lib.admm_sparse_l1class_run(h, C.byref(o), None, None))
        assert lib.admm_sparse_l1class_heldout(h, L.as_dp(one), L.as_dp(one), L.as_dp(one)) == L.E_INVALID
        assert "folds set" in lib.admm_last_error().decode()
        keep = [np.ascontiguousarray(fold, dtype=np.int32), np.array([0, 1, -1], dtype=np.int32)]
        L.check(lib.admm_sparse_l1class_set_folds(h, 3, ip(keep[0]), ip(keep[1])))
        L.check(lib.admm_sparse_l1class_run(h, C.byref(o), None, None))
        loss, err, wt = np.empty(3), np.empty(3), np.empty(3)
        L.check(lib.admm_sparse_l1class_heldout(h, L.as_dp(loss), L.as_dp(err), L.as_dp(wt)))
        assert list(wt) == [86.0, 86.0, 0.0] and loss[2] == 0.0 and err[2] == 0.0 and loss[0] > 0
    finally:
        lib.admm_sparse_l1class_destroy(h)
    with pytest.raises(ValueError, match="foldid has 5"):
        gpu.l1classifier_multi(c["D"], c["ell"], [0.1], dict(foldid=np.zeros(5), heldout=[0]))


# ---------------------------------------------------------------------------------------------- 6. l1classifier_cv
@pytest.mark.parametrize("measure", ("deviance", "class"))
def test_l1classifier_cv_end_to_end(gpu, measure):
    cv = W.cv_case(gpu)
    F, Lm = W.CV_FOLDS, W.CV_NLAMBDA
    m = cv["ell"].size
    o = dict(W.CV_LOOP, nfolds=F, seed=W.CV_SEED, cg_tol=W.CG_TOL, measure=measure)
    got = gpu.l1classifier_cv(cv["D"], cv["ell"], cv["lams"], o)
    assert np.array_equal(got["foldid"], cv["foldid"]) and np.array_equal(got["fold_lams"], cv["fold_lams"])
    for f in range(F):
        for l in range(Lm):
            assert int(got["fold_steps"][f, l]) == W.cv_fit(gpu, f, l)["steps"], (f, l)
    loss, err, wt = W.cv_sums(gpu)
    assert np.array_equal(got["heldout_weight"], wt) and np.array_equal(got["heldout_errors"], err)
    assert np.all(np.abs(got["heldout_loss"] - loss) <= LOSS_BOUND * loss)
    want = gpu.solvers.cv_summary(loss if measure == "deviance" else err, wt, cv["lams"])
    for key in ("index_min", "index_1se", "lam_min", "lam_1se"):
        assert got[key] == want[key], (key, got[key], want[key])
    _close("cvm", got["cvm"], want["cvm"], LOSS_BOUND)
    # every e_fl moves by at most LOSS_BOUND*e_fl and cvm by LOSS_BOUND*cvm: cvsd = ||v|| / sqrt(F - 1) with v_f =
    # sqrt(w_f / W)*(e_f - cvm) moves by at most LOSS_BOUND*2*max(e)/sqrt(F - 1) = sqrt(2)*LOSS_BOUND*max(e) for F = 3
    emax = np.max((loss if measure == "deviance" else err) / wt, axis=0)
    assert np.all(np.abs(got["cvsd"] - want["cvsd"]) <= np.sqrt(2.0) * LOSS_BOUND * emax)
    path = gpu.l1classifier_path(cv["D"], cv["ell"], cv["lams"], dict(W.CV_LOOP, cg_tol=W.CG_TOL))
    for key in ("xopt", "zopt", "uopt", "steps", "objopt", "df"):
        assert np.array_equal(got[key], path[key]), key  # the full-data path, in bits
    assert np.array_equal(got["cg_iters_total"][F * Lm:], path["cg_iters_total"])
    for l in range(Lm):
        ref = W.cv_fit(gpu, F, l)
        assert int(got["steps"][l]) == ref["steps"]
        _close(f"zopt[{l}]", got["zopt"][:, l], ref["zopt"], BOUND)
    assert got["measure"] == measure and got["df"][-1] > got["df"][0] and not got["cg_capped_updates"].any()


def test_the_tester(gpu):
    test = gpu.testers.sparsel1classifiercvtest(seed=1, rows=512, cols=96, density=0.1, nfolds=3, nlambda=5)
    print({k: test[k] for k in ("cvm", "lam_min", "lam_1se", "error_rate", "df", "weights_ok", "null_ok", "selects")})
    assert test["failed"] == 0
