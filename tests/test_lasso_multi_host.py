"""The multi-fit lasso on a dense design matrix without a device: the NumPy restatement of the loop with the
explicit inverse against the oracle's Cholesky loop (this also MEASURES the parity tolerance of test_gpu_lasso_multi), the
argument checks and refusals of the Python surface and of the C ABI that fire before the device is touched, the key set of
the results against a stub owner, and the automatic grid against the sparse caller's."""
import ctypes as C
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

import lasso_multi_restated as R


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_restatement_matches_the_oracle_and_measures_the_parity_gap(ap, shape, mode):
    """every fit, with nodualerror 0 and 1, every field (dnorm / derr included), no entry excluded"""
    c = R.case(ap, shape, mode)
    worst = 0.0
    for nd in (0, 1):
        steps = []
        for k in range(R.K):
            ref = R.oracle_fit(ap, shape, mode, k, nd)
            got = R.restated_fit(c, k, nd)
            assert got["steps"] == ref["steps"], (k, nd, got["steps"], ref["steps"])
            assert ("dnorm" in ref and not np.isnan(ref["dnorm"]).any()) == (nd == 0)
            gap = R.relgap(got, ref)
            print(f"{shape} {mode} nodualerror={nd} fit {k}: steps {ref['steps']}, gap {gap:.3e}")
            steps.append(ref["steps"])
            worst = max(worst, gap)
        # the oracle alone stops the fits at different iterations: the test of freezing
        assert len(set(steps)) >= 5, steps
    print(f"{shape} {mode}: largest gap {worst:.3e}")
    assert worst <= R.MEASURED_GAP, worst


def test_the_bound_follows_from_the_measurement():
    assert R.PARITY_BOUND == 10.0 * R.MEASURED_GAP and R.MEASURED_GAP <= 1e-7 and R.PARITY_BOUND <= 1e-6


def test_exact_cases_of_the_restated_loop(ap):
    """lambda = 0 from the zero start keeps u = 0.0 and z = x; lambda above lambda_max ends at z = 0.0"""
    c = R.case(ap, (200, 64), "shared")
    got = R.restated_fit(c, 0, 0)
    assert np.array_equal(got["zopt"], got["xopt"] + got["uopt"]) and not got["uopt"].any()
    got = R.restated_fit(c, 5, 0)
    assert not got["zopt"].any() and got["steps"] < 1000


def _problem(ap):
    c = R.case(ap, (200, 64), "shared")
    return c["A"], c["S"][:, 0]


# ------------------------------------------------------------------------------------------- the Python surface
@pytest.mark.parametrize("name,value", [("fast", 1), ("convtest", 1), ("relax", 1.5), ("adaptive", 1), ("xsolve", "cg"),
                                        ("xsolve", "pinv"), ("xsolve", 3), ("comm", object()), ("parallel", "both"),
                                        ("stopcond", "hnorm"), ("stopcond", "both")])
def test_options_refused_by_name_without_a_device(ap, name, value):
    D, s = _problem(ap)
    for call in (lambda: ap.lasso_multi_dense(D, s, [0.1, 0.2], {name: value}),
                 lambda: ap.lasso_path_dense(D, s, None, {name: value})):
        with pytest.raises(ValueError) as err:
            call()
        assert name in str(err.value), str(err.value)


def test_argument_checks_without_a_device(ap):
    D, s = _problem(ap)
    n = D.shape[1]
    with pytest.raises(ValueError, match="lasso_multi"):  # a sparse D belongs to the sparse callers
        ap.lasso_multi_dense(sp.csc_matrix(D), s, [0.1], {})
    with pytest.raises(ValueError, match="lasso_multi"):
        ap.lasso_path_dense(sp.csc_matrix(D), s, None, {})
    with pytest.raises(ValueError, match="fat lasso.*stays with lasso"):  # m < n
        ap.lasso_multi_dense(np.asfortranarray(D[:40]), s[:40], [0.1], {})
    with pytest.raises(ValueError, match="stays with lasso"):
        ap.lasso_path_dense(np.asfortranarray(D[:40]), s[:40], None, {})
    with pytest.raises(ValueError, match="rows"):
        ap.lasso_multi_dense(D, s[:-1], [0.1], {})
    with pytest.raises(ValueError, match="rows"):
        ap.lasso_path_dense(D, s[:-1], None, {})
    with pytest.raises(ValueError, match="at least one"):
        ap.lasso_multi_dense(D, s, [], {})
    with pytest.raises(ValueError, match="fit 1"):
        ap.lasso_multi_dense(D, s, [0.1, -0.2], {})
    with pytest.raises(ValueError, match="fit 1"):
        ap.lasso_multi_dense(D, s, [0.1, np.inf], {})
    with pytest.raises(ValueError, match="columns"):
        ap.lasso_multi_dense(D, np.zeros((200, 3)), [0.1, 0.2], {})
    with pytest.raises(ValueError, match="fit 0"):
        ap.lasso_multi_dense(D, s, [0.1, 0.2], dict(ridge=[-1.0, 0.0]))
    with pytest.raises(ValueError, match="ridge has 3"):
        ap.lasso_multi_dense(D, s, [0.1, 0.2], dict(ridge=[0.0, 0.0, 0.0]))
    with pytest.raises(ValueError, match="fit 1"):
        ap.lasso_multi_dense(D, s, [0.1, 0.2], dict(nonnegative=[0, 2]))
    with pytest.raises(ValueError, match="l1weights"):
        ap.lasso_multi_dense(D, s, [0.1], dict(l1weights=-np.ones(n)))
    with pytest.raises(ValueError, match="l1weights"):
        ap.lasso_multi_dense(D, s, [0.1], dict(l1weights=np.ones(n - 1)))
    for key in ("x0", "z0", "u0"):
        with pytest.raises(ValueError, match=key):
            ap.lasso_multi_dense(D, s, [0.1, 0.2], {key: np.zeros((n, 3))})
    with pytest.raises(ValueError, match="rho"):
        ap.lasso_multi_dense(D, s, [0.1], dict(rho=0.0))
    with pytest.raises(ValueError, match="nlambda"):
        ap.lasso_path_dense(D, s, None, dict(nlambda=0))
    with pytest.raises(ValueError, match="lambda_min_ratio"):
        ap.lasso_path_dense(D, s, None, dict(lambda_min_ratio=0.0))
    for xs in ("auto", "inverse", "trsv", "TRSV"):  # they pass the check: the next one fires
        with pytest.raises(ValueError, match="z0"):
            ap.lasso_multi_dense(D, s, [0.1], dict(xsolve=xs, z0=np.zeros(5)))
    with pytest.raises(TypeError):
        ap.lasso_multi_dense(D, s, [0.1], 3)


def test_lambda_max_and_the_log_grid_are_the_sparse_callers(ap, monkeypatch):
    """lasso_path_dense and lasso_path hand the same lambdas to their multi-fit callers for the same matrix"""
    D, s = _problem(ap)
    w = R.case(ap, (200, 64), "shared")["w"]
    seen = {}
    solvers = importlib.import_module(ap.__name__ + ".solvers")
    for name in ("lasso_multi", "lasso_multi_dense"):
        def fake(D_, s_, lams, options, name=name):
            seen.setdefault(name, []).append(np.array(lams))
            return dict(zopt=np.zeros((D_.shape[1], len(lams))))
        monkeypatch.setattr(solvers, name, fake)
    for o in ({}, dict(nlambda=7, lambda_min_ratio=0.05), dict(l1weights=w), dict(nlambda=1)):
        solvers.lasso_path_dense(D, s, None, dict(o))
        solvers.lasso_path(sp.csc_matrix(D), s, None, dict(o))
    for a, b, o in zip(seen["lasso_multi_dense"], seen["lasso_multi"], (10, 7, 10, 1)):
        assert a.shape == (o,) and np.allclose(a, b, rtol=1e-14, atol=0.0)  # (the sparse product's own summation order)
    g = np.abs(D.T @ s)
    assert seen["lasso_multi_dense"][0][0] == g.max()
    live = w > 0
    assert not live.all() and seen["lasso_multi_dense"][2][0] == (g[live] / w[live]).max()
    assert np.isclose(seen["lasso_multi_dense"][1][-1], 0.05 * g.max(), rtol=1e-14)


# ------------------------------------------------------------------------------------------- results against a stub
K3 = 3
STEPS = (2, 4, 1)


@pytest.fixture
def stubbed(ap, monkeypatch):
    made = []
    mod = importlib.import_module(ap.__name__ + ".lasso_multi")
    real = mod.LassoMulti

    class Stub(real):
        def __init__(self, D, S, lams, *args, **kw):
            self._h = None
            self.m, self.n = (int(v) for v in D.shape)
            self.K = len(lams)
            self.closed = False
            self.objevals = False
            self.made_with = kw
            made.append(self)

        @classmethod
        def chunk(cls):
            return 10

        def run(self, **kw):
            self.objevals = bool(kw.get("objevals", 0))
            self.dual = not kw.get("nodualerror", 0)
            self.xsolve = "inverse"
            self.ran_with = kw
            return dict(steps=np.array(STEPS, dtype=np.int64), stopped_early=np.ones(K3, dtype=np.int64),
                        objopt=np.arange(K3, dtype=np.float64) + 0.5, runtime=0.25)

        def fetch(self, field, rows):
            return np.asfortranarray(100.0 * field + np.arange(rows * K3, dtype=np.float64).reshape(rows, K3))

        def close(self):
            self.closed = True

    monkeypatch.setattr(mod, "LassoMulti", Stub)
    return made


_CORE = {"xopt", "zopt", "uopt", "steps", "pnorm", "perr", "objopt", "runtime", "solverruntime", "chunk", "lams", "xsolve"}


@pytest.mark.parametrize("nodual", (0, 1))
@pytest.mark.parametrize("objevals", (0, 1))
@pytest.mark.parametrize("caller", ("lasso_multi_dense", "lasso_path_dense"))
def test_result_keys_histories_and_close(ap, stubbed, caller, objevals, nodual):
    """lasso_multi's keys without nnz and the CG counters; xsolve names the form of the x-update"""
    D, s = _problem(ap)
    res = getattr(ap, caller)(D, s, [0.3, 0.2, 0.1], dict(objevals=objevals, nodualerror=nodual, rho=2.0, xsolve="trsv"))
    want = set(_CORE) | ({"df"} if caller == "lasso_path_dense" else set())
    if objevals:
        want.add("objevals")
    if not nodual:
        want |= {"dnorm", "derr"}
    assert set(res) == want, (sorted(set(res) - want), sorted(want - set(res)))
    for key in ("pnorm", "perr", "dnorm", "derr", "objevals"):
        if key in res:
            assert np.shape(res[key]) == (max(STEPS), K3), key
    assert len(stubbed) == 1 and stubbed[0].closed
    assert res["xsolve"] == "inverse" and res["chunk"] == 10 and res["runtime"] == 0.25
    assert res["xopt"].shape == res["zopt"].shape == res["uopt"].shape == (D.shape[1], K3)
    assert np.array_equal(res["lams"], [0.3, 0.2, 0.1]) and np.array_equal(res["steps"], STEPS)
    # rho goes to create and to the run; xsolve to create
    assert stubbed[0].made_with["rho"] == 2.0 and stubbed[0].made_with["xsolve"] == "trsv"
    assert stubbed[0].ran_with["rho"] == 2.0 and "cg_tol" not in stubbed[0].ran_with


# ------------------------------------------------------------------------------------------- the C ABI
def test_abi_symbols_structs_and_defaults(ap):
    L = ap._lib
    lib = L.load()
    for name in ("desc_default", "options_default", "create", "run", "fetch", "set_weights", "chunk", "destroy"):
        assert "admm_lasso_multi_" + name in L.EXPORTED_SYMBOLS and hasattr(lib, "admm_lasso_multi_" + name)
    assert "admm_op_symm_packed" in L.EXPORTED_SYMBOLS and hasattr(lib, "admm_op_symm_packed")
    d = L.LassoMultiDesc()
    lib.admm_lasso_multi_desc_default(C.byref(d))
    assert d.struct_size == C.sizeof(L.LassoMultiDesc) and (d.K, d.ns, d.rho, d.xsolve) == (1, 1, 1.0, L.XSOLVE_AUTO)
    o = L.LassoMultiOptions()
    lib.admm_lasso_multi_options_default(C.byref(o))
    assert o.struct_size == C.sizeof(L.LassoMultiOptions)
    assert (o.maxiters, o.rho, o.abstol, o.reltol, o.relax, o.nodualerror) == (1000, 1.0, 1e-5, 1e-3, 1.0, 0)
    assert C.sizeof(L.LassoMultiSummary) == 24
    assert ap.LassoMulti.chunk() == ap.SparseLassoMulti.chunk() == 10  # the layout is the sparse product's
    assert lib.admm_abi_version() == 5


def raw_create(L, D, S, lams, ns=1, ridge=None, nonneg=None, weights=None, comm=None, K=None, rho=None, xsolve=None,
               ldD=None):
    """admm_lasso_multi_create itself: (rc, handle)"""
    lib = L.load()
    d = L.LassoMultiDesc()
    lib.admm_lasso_multi_desc_default(C.byref(d))
    D = np.asfortranarray(D, dtype=np.float64)
    S = np.asfortranarray(S, dtype=np.float64)
    lam = np.ascontiguousarray(lams, dtype=np.float64)
    d.K, d.m, d.n, d.D, d.ldD = (lam.size if K is None else K), D.shape[0], D.shape[1], L.as_dp(D), D.shape[0]
    d.S, d.ns, d.lam = L.as_dp(S), ns, L.as_dp(lam)
    if ldD is not None:
        d.ldD = ldD
    keep = []
    for name, v in (("ridge", ridge), ("weights", weights)):
        if v is not None:
            keep.append(np.ascontiguousarray(v, dtype=np.float64))
            setattr(d, name, L.as_dp(keep[-1]))
    if nonneg is not None:
        keep.append(np.ascontiguousarray(nonneg, dtype=np.int32))
        d.nonneg = keep[-1].ctypes.data_as(C.POINTER(C.c_int32))
    if comm is not None:
        d.comm = comm
    if rho is not None:
        d.rho = rho
    if xsolve is not None:
        d.xsolve = xsolve
    h = C.c_void_p()
    rc = lib.admm_lasso_multi_create(C.byref(d), C.byref(h))
    return rc, h


def refusal_cases(L, c):
    """(name, expected code, message part, positional and keyword arguments of raw_create)"""
    D, S = c["A"], c["S"]
    lam = [0.1, 0.2, 0.3]
    w = np.ones(D.shape[1])
    return [("K = 0", L.E_INVALID, "K >= 1", (D, S, lam), dict(K=0)),
            ("ldD < m", L.E_INVALID, "ldD", (D, S, lam), dict(ldD=3)),
            ("ns = 2 for K = 3", L.E_INVALID, "columns", (D, np.zeros((D.shape[0], 2)), lam), dict(ns=2)),
            ("a negative lambda", L.E_INVALID, "fit 1: lambda", (D, S, [0.1, -0.2, 0.3]), {}),
            ("a NaN lambda", L.E_INVALID, "fit 2: lambda", (D, S, [0.1, 0.2, np.nan]), {}),
            ("an infinite ridge", L.E_INVALID, "fit 0: ridge", (D, S, lam), dict(ridge=[np.inf, 0.0, 0.0])),
            ("a negative ridge", L.E_INVALID, "fit 2: ridge", (D, S, lam), dict(ridge=[0.0, 0.0, -1.0])),
            ("nonneg 2", L.E_INVALID, "fit 1: nonneg", (D, S, lam), dict(nonneg=[0, 2, 0])),
            ("a negative weight", L.E_INVALID, "weight 4", (D, S, lam), dict(weights=np.where(np.arange(w.size) == 4, -1.0, w))),
            ("a NaN weight", L.E_INVALID, "weight 9", (D, S, lam), dict(weights=np.where(np.arange(w.size) == 9, np.nan, w))),
            ("rho = 0", L.E_INVALID, "rho", (D, S, lam), dict(rho=0.0)),
            ("xsolve = cg", L.E_UNSUPPORTED, "xsolve", (D, S, lam), dict(xsolve=L.XSOLVE_CG)),
            ("a communicator", L.E_UNSUPPORTED, "row-sharded", (D, S, lam), dict(comm=C.c_void_p(1))),
            ("m < n", L.E_UNSUPPORTED, "run lasso per fit", (D[:40], S[:40], lam), {})]


def test_abi_refusals_fire_before_the_device_is_touched(ap):
    """each of them returns its code with no handle on a machine without any device"""
    L = ap._lib
    c = R.case(ap, (200, 64), "shared")
    for name, code, part, args, kw in refusal_cases(L, c):
        rc, h = raw_create(L, *args, **kw)
        msg = L.load().admm_last_error().decode()
        assert rc == code and not h.value and part in msg, (name, rc, msg)


def test_operator_argument_checks(ap):
    L = ap._lib
    lib = L.load()
    M, X, Y = np.eye(4, order="F"), np.zeros((4, 2), order="F"), np.ones((4, 2), order="F")
    dp = L.as_dp
    assert lib.admm_op_symm_packed(None, 4, 4, dp(X), 2, None, dp(Y)) == L.E_INVALID
    assert lib.admm_op_symm_packed(dp(M), 0, 4, dp(X), 2, None, dp(Y)) == L.E_INVALID
    assert lib.admm_op_symm_packed(dp(M), 4, 3, dp(X), 2, None, dp(Y)) == L.E_INVALID
    assert lib.admm_op_symm_packed(dp(M), 4, 4, dp(X), 0, None, dp(Y)) == L.E_INVALID
    assert lib.admm_op_symm_packed(dp(M), 4, 4, None, 2, None, dp(Y)) == L.E_INVALID
