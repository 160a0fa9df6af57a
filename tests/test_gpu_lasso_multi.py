"""The multi-fit lasso on a dense design matrix on the device: the K runs over one cached inverse against
the oracle per fit in both modes and under both stop rules, two chunks with fits that stop at different iterations against
the same fits run alone (bits), the triangular-solve form, the objective, set_weights and a rerun, another rho, the
refusals that need an object, the path and its tester.

Parity bound.  The largest relative gap between the NumPy restatement (explicit inverse) and the oracle (Cholesky solves)
over these exact problems, fits, both stop rules and every field is 8.193e-12, measured by test_lasso_multi_host (the
1.25*lambda_max fit on 600x257, per-fit S); the bound here is 10x the recorded 8.2e-12 = 8.2e-11 -- the factor q37 - q39
use for the device's summation order inside the product -- and far below the project's 1e-6 parity definition.  The oracle
has the plain lasso only: the elastic-net fit under weights and the sign constraint is compared against the oracle's loop
with the restated prox (penalty_restated.run).  The l1 weights are shared by all fits of an object, so every problem runs
twice, all seven fits each time: without weights (fits 0 .. 5 are compared) and with them (fit 6 is)."""
import ctypes as C

import numpy as np
import pytest

import lasso_multi_restated as R
from test_gpu_sparse_lasso import _close

pytestmark = pytest.mark.gpu

BOUND = R.PARITY_BOUND
HIST = ("pnorm", "perr", "objevals")
KEYS = ("xopt", "zopt", "uopt", "pnorm", "perr", "dnorm", "derr", "objevals")
WORST = [0.0]


def _compare_fit(got, c, ref, dual, hist=HIST):
    """column c of a multi-fit result against one reference run: steps, every history over the fit's own steps, NaN
    beyond them, the three vectors and objopt"""
    assert int(got["steps"][c]) == ref["steps"], (c, got["steps"][c], ref["steps"])
    k = ref["steps"]
    for key in hist + (("dnorm", "derr") if dual else ()):
        _close(f"{key}[{c}]", got[key][:k, c], np.asarray(ref[key])[:k], BOUND)
        assert np.isnan(got[key][k:, c]).all()  # NaN past the fit's last step
    for key in ("xopt", "zopt", "uopt"):
        _close(f"{key}[{c}]", got[key][:, c], ref[key], BOUND)
    if "objevals" in hist:
        _close(f"objopt[{c}]", [got["objopt"][c]], [ref["objopt"]], BOUND)


def _multi(gpu, c, nodualerror, cols=None, weighted=False, lams=None, **more):
    """lasso_multi_dense on the case's D for the fits `cols` (default all seven) with their own starts"""
    cols = list(range(R.K)) if cols is None else list(cols)
    S = c["S"] if c["S"].shape[1] == 1 else np.asfortranarray(c["S"][:, cols])
    o = dict(R.loop_options(nodualerror), rho=R.RHO, z0=np.asfortranarray(c["z0"][:, cols]),
             u0=np.asfortranarray(c["u0"][:, cols]), ridge=[R.RIDGE[k] for k in cols],
             nonnegative=[R.NONNEG[k] for k in cols])
    if weighted:
        o["l1weights"] = c["w"]
    o.update(more)
    return gpu.lasso_multi_dense(c["A"], S, c["lams"][cols] if lams is None else lams, o)


# ---------------------------------------------------------------------------------------------- 1. parity per fit
@pytest.mark.parametrize("nodualerror", (0, 1))
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_fits_match_the_oracle_per_fit(gpu, shape, mode, nodualerror):
    c = R.case(gpu, shape, mode)
    dual = not nodualerror
    refs = [R.oracle_fit(gpu, shape, mode, k, nodualerror) for k in range(R.K)]
    assert len({r["steps"] for r in refs}) >= 5  # the fits stop at different iterations: the test of freezing
    got = _multi(gpu, c, nodualerror)
    assert got["xsolve"] == "inverse" and ("dnorm" in got) == dual and "nnz" not in got and "cg_iters_total" not in got
    assert np.array_equal(got["lams"], c["lams"]) and got["chunk"] == 10
    assert got["pnorm"].shape == (int(got["steps"].max()), R.K)
    for k in R.PLAIN:
        _compare_fit(got, k, refs[k], dual)
    # the exact cases inside the grid: lambda = 0 has z = x + u bit for bit, lambda above lambda_max has z = 0.0
    assert np.array_equal(got["zopt"][:, 0], got["xopt"][:, 0] + got["uopt"][:, 0])
    assert np.all(got["zopt"][:, 5] == 0.0)
    weighted = _multi(gpu, c, nodualerror, weighted=True)
    _compare_fit(weighted, R.FAMILY, refs[R.FAMILY], dual)
    assert np.all(weighted["zopt"][:, R.FAMILY] >= 0.0)


# ---------------------------------------------------------------------------------------------- 2. freezing, chunks
def test_twelve_fits_equal_the_same_fits_run_alone_in_bits(gpu):
    """K = 12 over two chunks, lambdas spread so that the fits stop at different iterations in both chunks: every fit has
    the bits of the same fit run alone, K = 1 -- a fit's numbers depend neither on its place nor on its neighbours"""
    shape = (300, 130)
    c = R.case(gpu, shape, "shared")
    lmax = float(c["lmax"][0])
    lams = lmax * np.array([0.01, 0.5, 0.02, 1.25, 0.05, 0.3, 0.1, 0.8, 0.2, 0.03, 0.015, 0.6])
    rng = np.random.default_rng(5)
    z0, u0 = (np.asfortranarray(0.1 * rng.standard_normal((130, 12))) for _ in range(2))
    o = dict(objevals=1, rho=R.RHO)
    got = gpu.lasso_multi_dense(c["A"], c["S"], lams, dict(o, z0=z0, u0=u0))
    steps = [int(s) for s in got["steps"]]
    print("steps", steps)
    assert len(set(steps[:10])) >= 5 and steps[10] != steps[11] and max(steps) < 1000
    for k in range(12):
        one = gpu.lasso_multi_dense(c["A"], c["S"], lams[k:k + 1],
                                    dict(o, z0=np.asfortranarray(z0[:, k:k + 1]), u0=np.asfortranarray(u0[:, k:k + 1])))
        assert int(one["steps"][0]) == steps[k]
        for key in KEYS:
            a, b = got[key][:, k], one[key][:, 0]
            if key not in ("xopt", "zopt", "uopt"):
                assert np.isnan(a[steps[k]:]).all()
                a = a[:steps[k]]
            assert np.array_equal(a.view(np.uint64), np.ascontiguousarray(b).view(np.uint64)), (k, key)
        assert got["objopt"][k] == one["objopt"][0]


# ---------------------------------------------------------------------------------------------- 3. the other forms
def test_triangular_solves_match_the_oracle(gpu):
    shape = (300, 130)
    c = R.case(gpu, shape, "perfit")
    got = _multi(gpu, c, 0, xsolve="trsv")
    assert got["xsolve"] == "trsv"
    for k in R.PLAIN:
        _compare_fit(got, k, R.oracle_fit(gpu, shape, "perfit", k, 0), True)


def test_objective_history_matches_the_oracle(gpu):
    """objevals = 1 on three tile rows: D X through the dense product per chunk, then the fit kernel"""
    shape = (600, 257)
    c = R.case(gpu, shape, "perfit")
    got = _multi(gpu, c, 0)
    for k in R.PLAIN:
        ref = R.oracle_fit(gpu, shape, "perfit", k, 0)
        _close(f"objevals[{k}]", got["objevals"][:ref["steps"], k], np.asarray(ref["objevals"])[:ref["steps"]], BOUND)
    off = _multi(gpu, c, 0, objevals=0)
    assert "objevals" not in off and np.isnan(off["objopt"]).all()
    for key in ("xopt", "zopt", "uopt", "pnorm", "dnorm"):  # the objective does not touch the iteration
        assert np.array_equal(off[key], got[key], equal_nan=True), key


def test_set_weights_and_a_second_run_on_the_same_object(gpu):
    shape = (200, 64)
    c = R.case(gpu, shape, "shared")
    cols = list(range(R.K))
    obj = gpu.LassoMulti(c["A"], c["S"], c["lams"], [R.RIDGE[k] for k in cols], [R.NONNEG[k] for k in cols], rho=R.RHO)
    try:
        run = dict(objevals=1, z0=c["z0"], u0=c["u0"])
        plain = obj.results(obj.run(**run))
        obj.set_weights(c["w"])
        weighted = obj.results(obj.run(**run))
        obj.set_weights(None)
        again = obj.results(obj.run(**run))
        with pytest.raises(gpu.AdmmError, match="weight 3"):
            obj.set_weights(np.where(np.arange(64) == 3, -1.0, 1.0))
    finally:
        obj.close()
    for k in R.PLAIN:
        _compare_fit(plain, k, R.oracle_fit(gpu, shape, "shared", k, 0), True)
    _compare_fit(weighted, R.FAMILY, R.oracle_fit(gpu, shape, "shared", R.FAMILY, 0), True)
    for key in KEYS:  # a run never depends on the one before it
        assert np.array_equal(again[key], plain[key], equal_nan=True), key


def test_a_second_object_with_another_rho(gpu):
    """rho belongs to the factor: an object built for rho = 2.5 agrees with the oracle at that rho"""
    shape = (200, 64)
    c = R.case(gpu, shape, "shared")
    from sparse_lasso_restated import oracle_run
    got = _multi(gpu, c, 0, cols=[1, 3], rho=2.5)
    for j, k in enumerate((1, 3)):
        ref = oracle_run(c["A"], R.response(c, k), float(c["lams"][k]), R.penalty_of(c, k, False),
                         R.fit_options(c, k, 0, rho=2.5))
        _compare_fit(got, j, ref, True)


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_run_time_refusals(gpu):
    c = R.case(gpu, (200, 64), "shared")
    L = gpu._lib
    obj = gpu.LassoMulti(c["A"], c["S"], c["lams"][:2], rho=1.0)
    try:
        for kw, code, part in ((dict(rho=2.0), L.E_INVALID, "differs from the rho the cached factor was built for"),
                               (dict(fast=L.FAST_OFF + 1), L.E_UNSUPPORTED, "fast / accelerated ADMM is not part of the multi-lasso loop"),
                               (dict(relax=1.5), L.E_UNSUPPORTED, "relaxation is not part of the multi-lasso loop"),
                               (dict(convtest=1), L.E_UNSUPPORTED, "convtest is not part of the multi-lasso loop")):
            with pytest.raises(gpu.AdmmError) as err:
                obj.run(**kw)
            assert err.value.code == code and part in str(err.value), str(err.value)
        ok = obj.results(obj.run())  # a refused run leaves the object usable
        assert ok["xopt"].shape == (64, 2) and int(ok["steps"].max()) < 1000
    finally:
        obj.close()


def test_a_fat_matrix_is_refused_naming_lasso(gpu):
    c = R.case(gpu, (200, 64), "shared")
    with pytest.raises(ValueError, match="stays with lasso"):
        gpu.lasso_multi_dense(np.asfortranarray(c["A"][:40]), c["S"][:40], [0.1], {})
    from test_lasso_multi_host import raw_create
    rc, h = raw_create(gpu._lib, c["A"][:40], c["S"][:40], [0.1])
    msg = gpu._lib.load().admm_last_error().decode()
    assert rc == gpu._lib.E_UNSUPPORTED and not h.value and "run lasso per fit" in msg


# ---------------------------------------------------------------------------------------------- 5. the path
def test_path_support_and_the_fit_at_lambda_max(gpu):
    shape = (600, 257)
    c = R.case(gpu, shape, "shared")
    got = gpu.lasso_path_dense(c["A"], c["S"][:, 0], None, dict(nlambda=12))
    lams = got["lams"]
    assert lams.shape == (12,) and lams[0] == c["lmax"][0] and np.all(np.diff(lams) < 0)
    df = [int(v) for v in got["df"]]
    print("df", df)
    assert all(b >= a for a, b in zip(df[:-1], df[1:]))  # non-increasing in lambda
    assert df[0] == 0 and np.all(got["zopt"][:, 0] == 0.0) and df[-1] > 0


def test_the_tester_passes(gpu):
    test = gpu.testers.lassopathtest(seed=0)
    assert test["failed"] == 0 and test["zero_above_lmax"] and test["support_grows"]
    assert test["results"]["xsolve"] in ("inverse", "trsv")
