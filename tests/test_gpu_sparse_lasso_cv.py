"""The sparse multi-lasso under observation weights and held-out folds, and lasso_cv, on the device: every
fit against the oracle on its own scaled row subset, the old bits of the fits that hold nothing out, the weighted
product as an operator, several row blocks, the edges, groups with folds, the cross-validation and the refusals.

Parity bound.  The largest relative gap between the NumPy restatement of the weighted loop (cg_tol = 1e-13) and the
oracle over these exact problems, both stop rules and every field is 2.789e-9, measured by test_sparse_lasso_cv_host
(fold 2 held out at 0.01*lambda_max on 257x65 under weights, nodualerror = 0); the bound here is 10x the recorded
2.8e-9 = 2.8e-8 -- the factor q37 .. q39 use for the device's summation order inside the products -- and below the
project's 1e-6 parity definition."""
import ctypes as C

import numpy as np
import pytest

import sparse_lasso_cv_restated as W
import sparse_lasso_restated as R
from sparse_cases import csc_of, desc_of, problem
from test_sparse_lasso_host import raw_create

pytestmark = pytest.mark.gpu

SMALL = (257, 65, 0.03)
BOUND = W.PARITY_BOUND
HIST = ("pnorm", "perr", "objevals")
FIELDS = ("xopt", "zopt", "uopt", "pnorm", "perr", "dnorm", "derr", "objevals")


def _close(name, got, ref, tol):
    got, ref = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(ref, dtype=np.float64))
    assert got.shape == ref.shape, f"{name}: shape {got.shape} vs {ref.shape}"
    assert not np.isnan(got).any() and not np.isnan(ref).any(), f"{name}: NaN"
    if ref.ndim == 1 and not name.split("[")[0].endswith("opt"):
        scale = np.maximum(np.abs(ref), 1e-12 + 1e-3 * np.max(np.abs(ref)))  # scalar histories: per entry
        err = float(np.max(np.abs(got - ref) / scale))
    else:
        err = float(np.max(np.abs(got - ref)) / max(1e-300, np.max(np.abs(ref))))
    print(f"{name}: relative error {err:.3e} (bound {tol:g})")
    assert err < tol, f"{name}: relative error {err:.3e} >= {tol:g}"


def _compare_fit(got, c, ref, dual):
    """test_gpu_sparse_lasso's comparison: steps, every history over the fit's own steps, NaN beyond them, the three
    vectors and objopt"""
    assert int(got["steps"][c]) == ref["steps"], (c, got["steps"][c], ref["steps"])
    k = ref["steps"]
    for key in HIST + (("dnorm", "derr") if dual else ()):
        _close(f"{key}[{c}]", got[key][:k, c], np.asarray(ref[key])[:k], BOUND)
        assert np.isnan(got[key][k:, c]).all()
    for key in ("xopt", "zopt", "uopt"):
        _close(f"{key}[{c}]", got[key][:, c], ref[key], BOUND)
    _close(f"objopt[{c}]", [got["objopt"][c]], [ref["objopt"]], BOUND)


def _multi(gpu, c, weighted, nodualerror, **more):
    o = dict(R.loop_options(nodualerror), cg_tol=1e-13, z0=c["z0"], u0=c["u0"], foldid=c["fold"], heldout=c["held"])
    if weighted:
        o["obsweights"] = c["obsw"]
    o.update(more)
    return gpu.lasso_multi(c["D"], c["s"], c["lams"][weighted], o)


def _check_heldout(got, c, weighted):
    """heldout_sse / heldout_weight against NumPy on the device's zopt: sums of squares, no cancellation"""
    for k, held in enumerate(c["held"]):
        sse, wt = W.heldout_sums(c["A"], c["s"], c["obsw"] if weighted else None, c["fold"], held, got["zopt"][:, k])
        assert abs(got["heldout_sse"][k] - sse) <= 1e-12 * sse, (k, got["heldout_sse"][k], sse)
        assert abs(got["heldout_weight"][k] - wt) <= 1e-12 * wt, (k, got["heldout_weight"][k], wt)
        if held < 0:
            assert got["heldout_sse"][k] == 0.0 and got["heldout_weight"][k] == 0.0


# ---------------------------------------------------------------------------------------------- 1. parity per fit
@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("nodualerror", (0, 1))
@pytest.mark.parametrize("shape", W.SHAPES)
def test_fits_match_the_oracle_on_their_own_rows(gpu, shape, nodualerror, weighted):
    c = W.case(gpu, shape)
    dual = not nodualerror
    refs = [W.oracle_fit(c, shape, k, weighted, nodualerror) for k in range(W.K)]
    assert len({r["steps"] for r in refs}) >= 5  # the fits stop at different iterations: the test of freezing
    got = _multi(gpu, c, weighted, nodualerror)
    assert got["xopt"].shape == (shape[1], W.K) and got["chunk"] == 10 and ("dnorm" in got) == dual
    for k in range(W.K):
        _compare_fit(got, k, refs[k], dual)
    for k in W.ZERO_FITS:
        assert np.all(got["zopt"][:, k] == 0.0)
    assert not got["cg_capped_updates"].any()
    _check_heldout(got, c, weighted)


# ---------------------------------------------------------------------------------------------- 2. the old bits
def _fetch_all(L, obj, summ, dual=True):
    S = int(summ["steps"].max())
    fields = [(L.SLM_F_XOPT, obj.n), (L.SLM_F_ZOPT, obj.n), (L.SLM_F_UOPT, obj.n), (L.SLM_F_PNORM, S),
              (L.SLM_F_PERR, S), (L.SLM_F_OBJEVALS, S)] + ([(L.SLM_F_DNORM, S), (L.SLM_F_DERR, S)] if dual else [])
    return [summ["steps"], summ["objopt"], summ["cg_iters_total"], summ["cg_capped_updates"]] + \
           [obj.fetch(f, r) for f, r in fields]


def test_fits_that_hold_nothing_out_keep_the_old_bits(gpu):
    """without obsweights the heldout = -1 fits of a mixed object are the fits of lasso_multi without the options"""
    c = W.case(gpu, SMALL)
    lams = c["lams"][False]
    held = np.array([-1, 0, -1, 1, 2, -1, 0, -1, 1, -1, -1, 2, -1])
    o = dict(objevals=1, cg_tol=1e-13, z0=c["z0"], u0=c["u0"])
    mixed = gpu.lasso_multi(c["D"], c["s"], lams, dict(o, foldid=c["fold"], heldout=held))
    plain = gpu.lasso_multi(c["D"], c["s"], lams, o)
    full = np.flatnonzero(held < 0)
    S = int(plain["steps"].max())
    assert np.array_equal(mixed["steps"][full], plain["steps"][full]) and "heldout_sse" not in plain
    for key in FIELDS:
        rows = slice(None) if key.endswith("opt") else slice(0, min(S, mixed[key].shape[0]))
        for k in full:
            st = None if key.endswith("opt") else int(plain["steps"][k])
            assert np.array_equal(mixed[key][rows, k][:st], plain[key][rows, k][:st]), (key, k)
    for key in ("objopt", "cg_iters_total", "cg_capped_updates"):
        assert np.array_equal(mixed[key][full], plain[key][full]), key
    assert not np.array_equal(mixed["xopt"][:, 1], plain["xopt"][:, 1])


def test_set_observations_none_restores_the_unweighted_bits(gpu):
    L = gpu._lib
    c = W.case(gpu, SMALL)
    obj = gpu.SparseLassoMulti(c["D"], c["s"], c["lams"][True])
    try:
        go = lambda: _fetch_all(L, obj, obj.run(objevals=1, maxiters=40, z0=c["z0"], u0=c["u0"]))
        plain = go()
        with pytest.raises(gpu.AdmmError) as err:  # no observations behind the run
            obj.heldout()
        assert err.value.code == L.E_INVALID
        obj.set_observations(c["obsw"], c["fold"], c["held"])
        weighted = go()
        sums = obj.heldout()
        assert not np.array_equal(plain[4], weighted[4])
        for bad, part in ((dict(obsweights=np.where(np.arange(257) == 3, -1.0, 1.0)), "weight 3"),
                          (dict(fold=np.where(np.arange(257) == 9, -1, c["fold"]), heldout=c["held"]), "row 9")):
            with pytest.raises(gpu.AdmmError) as err:  # a refused call changes nothing
                obj.set_observations(**bad)
            assert err.value.code == L.E_INVALID and part in str(err.value)
        again = go()
        assert all(np.array_equal(a, b) for a, b in zip(sums, obj.heldout()))
        obj.set_observations(None, None, None)
        restored = go()
        with pytest.raises(gpu.AdmmError):
            obj.heldout()
    finally:
        obj.close()
    for a, b in zip(weighted, again):
        assert np.array_equal(a, b, equal_nan=True)
    for a, b in zip(plain, restored):
        assert np.array_equal(a, b, equal_nan=True)


# ---------------------------------------------------------------------------------------------- 3. the operator
def _op_weighted(L, csc, X, obsw, nfolds, fold, held):
    lib = L.load()
    m, K = csc.shape[0], X.shape[1]
    Y = np.full((m, K), np.nan, order="F")
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.int32) for a in (fold, held)]
    w = None if obsw is None else np.ascontiguousarray(obsw, dtype=np.float64)
    rc = lib.admm_op_spmm_weighted(C.byref(desc_of(L, csc)), K, L.as_dp(X), None if w is None else L.as_dp(w), nfolds,
                                   None if keep[0] is None else keep[0].ctypes.data_as(C.POINTER(C.c_int32)),
                                   None if keep[1] is None else keep[1].ctypes.data_as(C.POINTER(C.c_int32)), L.as_dp(Y))
    return rc, Y


@pytest.mark.parametrize("with_weights", (False, True))
def test_the_weighted_product_as_an_operator(gpu, with_weights):
    """257 x 65 (row 3 dense, row 5 empty, the last workgroup partial), K = 11: two chunks, nine padding columns"""
    L = gpu._lib
    lib = L.load()
    p = problem(gpu, 257, 65, 0.03, seed=1)
    A, csc = p["A"], csc_of(p["D"])
    assert np.count_nonzero(A[3]) >= 60 and not A[5].any()
    rng = np.random.default_rng(31)
    K, nfolds = 11, 4
    fold = rng.permutation(257) % nfolds
    held = np.array([0, 1, 2, 3, -1, 0, 1, 2, 3, -1, 2])
    obsw = rng.uniform(0.5, 2.0, 257) if with_weights else None
    if with_weights:
        obsw[[2, 128]] = 0.0
    X = np.asfortranarray(rng.standard_normal((65, K)))
    # a row of X that only a held-out row of D reads: column j of D is nonzero in rows of fold 0 alone
    j = 20
    fold[A[:, j] != 0.0] = 0
    fold[3] = 0  # (the dense row reads every row of X)
    only0 = [k for k in range(K) if held[k] == 0]
    Xn = X.copy(order="F")
    Xn[j, only0] = np.nan
    Y0 = np.empty((257, K), order="F")
    assert lib.admm_op_spmm(C.byref(desc_of(L, csc)), 0, K, L.as_dp(X), L.as_dp(Y0)) == L.OK
    rc, Y = _op_weighted(L, csc, Xn, obsw, nfolds, fold, held)
    assert rc == L.OK, lib.admm_last_error()  # (the operator checks the padding columns itself: they stay +0.0)
    w = np.ones(257) if obsw is None else obsw
    for k in range(K):
        out = fold == held[k]
        assert out.any() == (held[k] >= 0)
        assert np.array_equal(Y[~out, k], Y0[~out, k] * w[~out]), k  # one rounding, as NumPy's product
        assert np.all(Y[out, k] == 0.0) and not np.signbit(Y[out, k]).any(), k  # +0.0 whatever acc holds (NaN here)
    assert not np.isnan(Y).any() and np.all(Y[5] == 0.0) and not np.signbit(Y[5]).any()
    # the select, not a product: without it the planted NaN would come through
    rc, Yall = _op_weighted(L, csc, Xn, obsw, nfolds, fold, np.full(K, -1))
    assert rc == L.OK and np.isnan(Yall[np.ix_(A[:, j] != 0.0, only0)]).all()


# ---------------------------------------------------------------------------------------------- 4. several row blocks
@pytest.mark.parametrize("shape,maxiters", [(W.TALL, W.TALL_MAXITERS), (W.WIDE, W.WIDE_MAXITERS)])
def test_a_workgroup_takes_several_row_blocks(gpu, shape, maxiters):
    """8200 x 40 with objevals = 1: the weighted fit kernel and the epilogue past 32 * 256 rows; 60 x 8300: the per-fit
    D's in the element pass"""
    c = W.big_case(gpu, shape)
    assert max(c["A"].shape) > 32 * 256
    got = _multi(gpu, c, True, 0, maxiters=maxiters)
    for k in range(len(c["held"])):
        _compare_fit(got, k, W.oracle_fit(c, shape, k, True, 0, maxiters=maxiters), dual=True)
    _check_heldout(got, c, True)


# ---------------------------------------------------------------------------------------------- 5. edges
def test_a_fold_that_holds_out_every_row(gpu):
    c = W.case(gpu, SMALL)
    got = gpu.lasso_multi(c["D"], c["s"], [0.3, 0.3, 0.3],
                          dict(objevals=1, foldid=np.zeros(257, dtype=int), heldout=[-1, 0, -1]))
    assert np.all(got["xopt"][:, 1] == 0.0) and np.all(got["zopt"][:, 1] == 0.0) and np.all(got["uopt"][:, 1] == 0.0)
    assert int(got["steps"][1]) == 1 and int(got["cg_iters_total"][1]) == 0 and got["objopt"][1] == 0.0
    assert int(got["steps"][0]) > 1 and np.array_equal(got["xopt"][:, 0], got["xopt"][:, 2])
    assert got["heldout_weight"][1] == 257.0 and got["heldout_weight"][0] == 0.0 and got["heldout_sse"][0] == 0.0
    assert abs(got["heldout_sse"][1] - float(c["s"] @ c["s"])) <= 1e-12 * float(c["s"] @ c["s"])


def test_a_fold_that_empties_a_column(gpu):
    c = W.emptied_case(gpu)
    got = _multi(gpu, c, False, 0)
    for k in range(len(c["held"])):
        _compare_fit(got, k, W.oracle_fit(c, "emptied", k, False, 0), dual=True)
    assert not got["cg_capped_updates"].any()


def test_rerun_and_check_every_give_the_same_bits(gpu):
    L = gpu._lib
    c = W.case(gpu, SMALL)
    obj = gpu.SparseLassoMulti(c["D"], c["s"], c["lams"][True])
    try:
        obj.set_observations(c["obsw"], c["fold"], c["held"])
        runs = []
        for ce in (0, 0, 1, 8):
            summ = obj.run(objevals=1, check_every=ce, cg_tol=1e-13, z0=c["z0"], u0=c["u0"])
            runs.append(_fetch_all(L, obj, summ) + list(obj.heldout()))
        assert len(set(runs[0][0])) >= 5
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert a.size > 0 and np.array_equal(a, b, equal_nan=True)
    finally:
        obj.close()


# ---------------------------------------------------------------------------------------------- 6. groups with folds
def test_groups_with_folds_match_the_row_subset(gpu):
    import scipy.sparse as sp
    c = W.case(gpu, SMALL)
    sizes = [5] * 13
    lam = 0.05 * float(np.max(np.abs(c["A"].T @ c["s"])))
    o = dict(objevals=1, cg_tol=1e-13, l1=[0.2 * lam] * 3)
    got = gpu.grouplasso_multi(c["D"], c["s"], [lam] * 3, sizes, dict(o, foldid=c["fold"], heldout=[0, 1, 2]))
    for f in range(3):
        rows = c["fold"] != f
        ref = gpu.grouplasso_multi(sp.csc_matrix(c["A"][rows]), c["s"][rows], [lam], sizes, dict(o, l1=[0.2 * lam]))
        assert int(got["steps"][f]) == int(ref["steps"][0])
        k = int(ref["steps"][0])
        for key in FIELDS:
            a, b = (got[key][:, f], ref[key][:, 0]) if key.endswith("opt") else (got[key][:k, f], ref[key][:k, 0])
            _close(f"{key}[fold {f}]", a, b, BOUND)
        _close(f"objopt[fold {f}]", [got["objopt"][f]], [ref["objopt"][0]], BOUND)
    _check_heldout(got, dict(c, held=[0, 1, 2]), False)


# ---------------------------------------------------------------------------------------------- 7. lasso_cv
def test_lasso_cv_against_the_oracle_and_the_path(gpu):
    cv = W.cv_case(gpu)
    F, Lm = W.CV_FOLDS, W.CV_NLAMBDA
    o = dict(objevals=1, nfolds=F, foldid=cv["foldid"])
    got = gpu.lasso_cv(cv["D"], cv["s"], cv["lams"], o)
    assert np.array_equal(got["lams"], cv["lams"]) and np.array_equal(got["foldid"], cv["foldid"])
    assert np.array_equal(got["fold_lams"], cv["fold_lams"])  # lambda_l * (training weight / total weight)
    sse, wt = np.zeros((F, Lm)), np.zeros((F, Lm))
    for f in range(F):
        for l in range(Lm):
            ref = W.cv_oracle(gpu, f, l)
            assert int(got["fold_steps"][f, l]) == ref["steps"], (f, l)
            sse[f, l], wt[f, l] = W.heldout_sums(cv["A"], cv["s"], None, cv["foldid"], f, ref["zopt"])
    want = gpu.solvers.cv_summary(sse, wt, cv["lams"])
    for key in ("index_min", "index_1se", "lam_min", "lam_1se"):
        assert got[key] == want[key], (key, got[key], want[key])
    tol = BOUND * W.CV_CONDITION
    _close("cvm", got["cvm"], want["cvm"], tol)
    assert np.all(np.abs(got["cvsd"] - want["cvsd"]) <= tol * want["cvm"])
    assert np.array_equal(got["heldout_weight"], wt) and got["heldout_sse"].shape == (F, Lm)
    path = gpu.lasso_path(cv["D"], cv["s"], cv["lams"], dict(objevals=1))
    for key in ("xopt", "zopt", "uopt", "steps", "objopt", "df"):
        assert np.array_equal(got[key], path[key]), key
    assert np.array_equal(got["cg_iters_total"][F * Lm:], path["cg_iters_total"])
    for l in range(Lm):
        _compare_full = W.cv_oracle(gpu, F, l)
        assert int(got["steps"][l]) == _compare_full["steps"]
        _close(f"zopt[full {l}]", got["zopt"][:, l], _compare_full["zopt"], BOUND)
    off = gpu.lasso_cv(cv["D"], cv["s"], cv["lams"], dict(o, scale_lambda=0))
    assert np.array_equal(off["fold_lams"], np.repeat(cv["lams"][None, :], F, axis=0))
    assert not np.array_equal(off["heldout_sse"], got["heldout_sse"])
    assert np.array_equal(off["xopt"], got["xopt"])  # the full-data fits do not move
    auto = gpu.lasso_cv(cv["D"], cv["s"], None, dict(nfolds=F, nlambda=4))
    assert auto["lams"].shape == (4,) and auto["lams"][0] == float(np.max(np.abs(cv["D"].T @ cv["s"])))
    assert np.array_equal(auto["foldid"], gpu.solvers.cv_folds(600, F, 0)) and auto["cvm"].shape == (4,)


def test_sparse_lasso_cv_tester_passes(gpu):
    t = gpu.testers.sparselassocvtest(seed=0, rows=1024, cols=256, density=0.05, nfolds=3, nlambda=6)
    assert t["failed"] == 0 and t["weights_ok"] and t["null_ok"] and t["selects"], (t["cvm"], t["df"])
    assert t["results"]["heldout_sse"].shape == (3, 6) and t["df"][0] == 0 and t["null_fits"] >= 2


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_through_the_c_abi(gpu):
    """each returns ADMM_E_INVALID with its culprit named, and a well-formed call succeeds right behind it"""
    L = gpu._lib
    lib = L.load()
    c = W.case(gpu, SMALL)
    csc = csc_of(c["D"])
    rc, h = raw_create(L, csc, c["s"].reshape(-1, 1), [0.1, 0.2, 0.3])
    assert rc == L.OK and h.value, lib.admm_last_error()
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    fold, held, ones = i32(c["fold"]), i32([0, -1, 2]), np.ones(257)
    cases = [("a negative weight", np.where(np.arange(257) == 4, -1.0, ones), 3, fold, held, "weight 4"),
             ("a NaN weight", np.where(np.arange(257) == 9, np.nan, ones), 3, fold, held, "weight 9"),
             ("an infinite weight", np.where(np.arange(257) == 11, np.inf, ones), 0, None, None, "weight 11"),
             ("nfolds = 0", None, 0, fold, held, "nfolds"),
             ("a fold id past nfolds", None, 2, fold, i32([0, -1, 1]), "row "),
             ("a negative fold id", None, 3, i32(np.where(np.arange(257) == 6, -1, c["fold"])), held, "row 6"),
             ("heldout = nfolds", None, 3, fold, i32([0, 3, 2]), "fit 1"),
             ("heldout = -2", None, 3, fold, i32([0, -1, -2]), "fit 2"),
             ("heldout without fold", None, 3, None, held, "heldout")]
    sse, wt = np.empty(3), np.empty(3)
    try:
        assert lib.admm_sparse_lasso_heldout(h, L.as_dp(sse), L.as_dp(wt)) == L.E_INVALID  # before a run
        o = L.SparseLassoOptions()
        lib.admm_sparse_lasso_options_default(C.byref(o))
        o.maxiters = 5
        assert lib.admm_sparse_lasso_run(h, C.byref(o), None, None) == L.OK
        assert lib.admm_sparse_lasso_heldout(h, L.as_dp(sse), L.as_dp(wt)) == L.E_INVALID  # without observations
        assert "observations" in lib.admm_last_error().decode()
        for name, w, nfolds, f, hd, part in cases:
            w = None if w is None else np.ascontiguousarray(w)
            rc = lib.admm_sparse_lasso_set_observations(h, None if w is None else L.as_dp(w), nfolds, ip(f), ip(hd))
            msg = lib.admm_last_error().decode()
            assert rc == L.E_INVALID and part in msg, (name, rc, msg)
            rc2, _ = _op_weighted(L, csc, np.ones((65, 3), order="F"), w, nfolds, f, hd)  # the operator's own checks
            assert rc2 == L.E_INVALID and part in lib.admm_last_error().decode(), name
            assert lib.admm_sparse_lasso_set_observations(h, L.as_dp(ones), 3, ip(fold), ip(held)) == L.OK, name
        assert lib.admm_sparse_lasso_run(h, C.byref(o), None, None) == L.OK
        assert lib.admm_sparse_lasso_heldout(h, L.as_dp(sse), L.as_dp(wt)) == L.OK
        assert wt[1] == 0.0 and wt[0] == float(np.sum(c["fold"] == 0)) and sse[0] > 0.0
        assert lib.admm_sparse_lasso_heldout(h, None, L.as_dp(wt)) == L.E_INVALID
    finally:
        lib.admm_sparse_lasso_destroy(h)


@pytest.mark.parametrize("key", ("obsweights", "foldid", "heldout"))
def test_the_dense_solvers_refuse_the_options_by_name(gpu, key):
    c = W.case(gpu, SMALL)
    value = dict(obsweights=np.ones(257), foldid=c["fold"], heldout=np.array([0, -1]))[key]
    for call in (gpu.lasso_multi_dense, gpu.lasso_path_dense):
        with pytest.raises(ValueError) as err:
            call(c["A"], c["s"], [0.1, 0.2], {key: value})
        assert f"options.{key}" in str(err.value)
    ok = gpu.lasso_multi_dense(c["A"], c["s"], [0.1, 0.2], {})
    assert ok["xopt"].shape == (65, 2)
