"""The multi-fit lasso on a sparse design matrix on the device: the K lock-step runs against the oracle per
fit in both modes and under both stop rules, the exact cases, the single-fit engine, two chunks, a workgroup with several
row blocks in the element pass (n > 8192) and in the fit kernel (m > 8192), rank-deficient matrices, freezing, the
reported iteration cap, reruns, weights, the path and its tester, refusals.

Parity bound.  The largest relative gap between the NumPy restatement (cg_tol = 1e-13) and the oracle over these exact
problems, fits, both stop rules and every field is 5.803e-10, measured by test_sparse_lasso_host (the 0.01*lambda_max fit
on 80x200, per-fit S, nodualerror = 0); the bound here is 10x the recorded 5.9e-10 = 5.9e-9 -- the factor q37 and q38
use for the device's summation order inside the products -- and below the project's 1e-6 parity definition.  The oracle
has the plain lasso only: the elastic-net fit under weights and the sign constraint is compared against the oracle's loop
with the restated prox (penalty_restated.run), as test_gpu_penalty does.  The l1 weights are shared by all fits of an
object, so every problem runs twice, all seven fits each time: without weights (fits 0 .. 5 are compared) and with them
(fit 6 is)."""
import ctypes as C

import numpy as np
import pytest

import sparse_lasso_restated as R
from sparse_cases import csc_of
from test_sparse_lasso_host import raw_create, refusal_cases

pytestmark = pytest.mark.gpu

SMALL = (257, 65, 0.03)
BOUND = R.PARITY_BOUND
HIST = ("pnorm", "perr", "objevals")


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
    """column c of a multi-fit result against one reference run: steps, every history over the fit's own steps, NaN
    beyond them, the three vectors and objopt"""
    assert int(got["steps"][c]) == ref["steps"], (c, got["steps"][c], ref["steps"])
    k = ref["steps"]
    for key in HIST + (("dnorm", "derr") if dual else ()):
        _close(f"{key}[{c}]", got[key][:k, c], np.asarray(ref[key])[:k], BOUND)
        assert np.isnan(got[key][k:, c]).all()  # NaN past the fit's last step
    for key in ("xopt", "zopt", "uopt"):
        _close(f"{key}[{c}]", got[key][:, c], ref[key], BOUND)
    _close(f"objopt[{c}]", [got["objopt"][c]], [ref["objopt"]], BOUND)


def _multi(gpu, c, nodualerror, cols=None, weighted=False, **more):
    """lasso_multi on the case's sparse D for the fits `cols` (default all seven) with their own starts"""
    cols = list(range(R.K)) if cols is None else list(cols)
    S = c["S"] if c["S"].shape[1] == 1 else np.asfortranarray(c["S"][:, cols])
    o = dict(R.loop_options(nodualerror), cg_tol=1e-13, z0=np.asfortranarray(c["z0"][:, cols]),
             u0=np.asfortranarray(c["u0"][:, cols]), ridge=[R.RIDGE[k] for k in cols],
             nonnegative=[R.NONNEG[k] for k in cols])
    if weighted:
        o["l1weights"] = c["w"]
    o.update(more)
    return gpu.lasso_multi(c["D"], S, c["lams"][cols], o)


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
    assert got["xsolve"] == "cg" and got["nnz"] == c["D"].nnz and ("dnorm" in got) == dual
    assert np.array_equal(got["lams"], c["lams"]) and got["chunk"] == 10
    assert got["pnorm"].shape == (int(got["steps"].max()), R.K)
    for k in R.PLAIN:
        _compare_fit(got, k, refs[k], dual)
    assert not got["cg_capped_updates"].any() and np.all(got["cg_iters_total"] >= got["steps"])
    # the exact cases inside the grid: lambda = 0 has z = x + u bit for bit, lambda above lambda_max has z = 0.0
    assert np.array_equal(got["zopt"][:, 0], got["xopt"][:, 0] + got["uopt"][:, 0])
    assert np.all(got["zopt"][:, 5] == 0.0)
    weighted = _multi(gpu, c, nodualerror, weighted=True)
    _compare_fit(weighted, R.FAMILY, refs[R.FAMILY], dual)
    assert np.all(weighted["zopt"][:, R.FAMILY] >= 0.0)


def test_lambda_zero_from_any_start_keeps_z_equal_to_x_plus_u(gpu):
    """tau = 0 and kappa = 1: the prox returns x + u bit for bit, whatever the start"""
    c = R.case(gpu, SMALL, "shared")
    rng = np.random.default_rng(11)
    z0, u0 = (np.asfortranarray(rng.standard_normal((65, 1))) for _ in range(2))
    got = gpu.lasso_multi(c["D"], c["S"], [0.0], dict(maxiters=1, z0=z0, u0=u0))
    # after one iteration u = u0 + (x - z) and z = x + u0: z is recovered from x and u0 alone
    assert np.array_equal(got["zopt"][:, 0], got["xopt"][:, 0] + u0[:, 0]) and got["zopt"].any()


def test_a_zero_response_gives_x_exactly_zero_in_one_step(gpu):
    c = R.case(gpu, SMALL, "shared")
    S = np.asfortranarray(np.column_stack([c["S"][:, 0], np.zeros(257), c["S"][:, 0]]))
    got = gpu.lasso_multi(c["D"], S, [0.3, 0.3, 0.3], dict(objevals=1))
    assert np.all(got["xopt"][:, 1] == 0.0) and np.all(got["zopt"][:, 1] == 0.0) and np.all(got["uopt"][:, 1] == 0.0)
    assert int(got["steps"][1]) == 1 and int(got["cg_iters_total"][1]) == 0 and got["objopt"][1] == 0.0
    assert int(got["steps"][0]) > 1 and np.array_equal(got["xopt"][:, 0], got["xopt"][:, 2])


# ---------------------------------------------------------------------------------------------- 2. the engine
def test_one_column_matches_lasso_on_the_sparse_engine(gpu):
    """lasso(<sparse D>) keeps running on the engine (q35: one-column SpMV, its own CG); the same fit through the new
    object agrees with it at the parity bound"""
    c = R.case(gpu, SMALL, "shared")
    k = 3
    one = gpu.lasso(c["D"], c["S"][:, 0], float(c["lams"][k]),
                    dict(objevals=1, cg_tol=1e-13, z0=c["z0"][:, k], u0=c["u0"][:, k]))
    got = _multi(gpu, c, 0, [k])
    assert one["xsolve"] == "cg" and "xvals" in one  # the engine's own result, histories and all
    _compare_fit(got, 0, one, dual=True)


# ---------------------------------------------------------------------------------------------- 3. chunks
def test_two_chunks(gpu):
    """K = Kc + 1 with the last fit a duplicate of fit 0: bitwise equal columns; K = Kc and K = 1 give the same bits"""
    c = R.case(gpu, SMALL, "shared")
    kc = gpu.SparseLassoMulti.chunk()
    assert kc == 10
    cols = [k % R.K for k in range(kc)] + [0]
    got = _multi(gpu, c, 0, cols)
    assert got["xopt"].shape == (65, kc + 1) and got["chunk"] == kc
    for k in (0, kc):
        _compare_fit(got, k, R.oracle_fit(gpu, SMALL, "shared", 0, 0), dual=True)
    keys = ("xopt", "zopt", "uopt", "pnorm", "perr", "dnorm", "derr", "objevals")
    for key in keys:
        assert np.array_equal(got[key][:, kc], got[key][:, 0], equal_nan=True), key
        assert np.array_equal(got[key][:, 7], got[key][:, 0], equal_nan=True), key
    ten = _multi(gpu, c, 0, cols[:kc])
    one = _multi(gpu, c, 0, [0])
    S1 = int(one["steps"][0])
    for key in keys:
        assert np.array_equal(ten[key], got[key][:, :kc], equal_nan=True), key
        rows = S1 if key in keys[3:] else None
        assert np.array_equal(one[key][:, 0], got[key][:rows, 0]), key
    assert np.array_equal(ten["cg_iters_total"], got["cg_iters_total"][:kc])


# ---------------------------------------------------------------------------------------------- 4. several row blocks
@pytest.mark.parametrize("shape,fits,maxiters", [(R.WIDE, R.WIDE_FITS, R.WIDE_MAXITERS),
                                                 (R.TALL, R.TALL_FITS, R.TALL_MAXITERS)])
def test_a_workgroup_takes_several_row_blocks(gpu, shape, fits, maxiters):
    """60 x 8300: the n-length element pass and CG kernels; 8200 x 40 with objevals = 1: the m-length fit kernel
    (the CG kernels' own row-block edges, one solve at a time: test_gpu_spmm_cg.test_row_block_edges)"""
    c = R.big_case(gpu, shape)
    assert max(c["A"].shape) > 32 * 256
    got = _multi(gpu, c, 0, fits, maxiters=maxiters)
    for i, k in enumerate(fits):
        _compare_fit(got, i, R.big_oracle(gpu, shape, k, maxiters), dual=True)
        rest = R.restated_fit(c, k, 0, weighted=False, maxiters=maxiters)
        _compare_fit(got, i, rest, dual=True)


# ---------------------------------------------------------------------------------------------- 5. rank deficiency
def test_rank_deficient_matrices_match_the_oracle(gpu):
    """the empty column 7 and a duplicate of column 9 in its place: rho > 0 keeps the oracle's Cholesky"""
    A = R.matrix(gpu, *SMALL)
    assert not A[:, 7].any()
    B = A.copy()
    B[:, 7] = B[:, 9]
    assert np.linalg.matrix_rank(B) == 64
    for M, cols in ((A, [1, 3]), (B, [2, 4])):
        c = R.case(gpu, SMALL, "shared", A=np.asfortranarray(M))
        got = _multi(gpu, c, 0, cols)
        for i, k in enumerate(cols):
            ref = R.oracle_run(c["A"], R.response(c, k), float(c["lams"][k]), R.penalty_of(c, k, False),
                               R.fit_options(c, k, 0))
            _compare_fit(got, i, ref, dual=True)
        assert not got["cg_capped_updates"].any()


# ---------------------------------------------------------------------------------------------- 6. freezing
def test_a_stopped_fit_is_frozen(gpu):
    """fit 3 stops long before the fit above lambda_max does: its x, z, u are those of its own run"""
    c = R.case(gpu, SMALL, "shared")
    got = _multi(gpu, c, 0)
    alone = _multi(gpu, c, 0, [3])
    assert int(alone["steps"][0]) == int(got["steps"][3]) < int(got["steps"].max()) - 50
    for key in ("xopt", "zopt", "uopt"):
        assert np.array_equal(alone[key][:, 0], got[key][:, 3]), key
    S3 = int(alone["steps"][0])
    for key in HIST + ("dnorm", "derr"):
        assert np.array_equal(alone[key][:, 0], got[key][:S3, 3]), key


# ---------------------------------------------------------------------------------------------- 7. the cap
def test_the_iteration_cap_is_reported(gpu):
    c = R.case(gpu, (600, 120, 0.05), "shared")
    got = _multi(gpu, c, 0, maxiters=30, cg_maxit=2)
    assert np.all(got["steps"] >= 1) and np.isfinite(got["xopt"]).all()
    assert got["cg_capped_updates"].shape == (R.K,) and np.all(got["cg_capped_updates"] > 0)
    assert np.all(got["cg_iters_total"] <= 2 * got["steps"])


# ---------------------------------------------------------------------------------------------- 8. same bits
def _fetch_all(L, obj, summ, dual):
    S = int(summ["steps"].max())
    fields = [(L.SLM_F_XOPT, obj.n), (L.SLM_F_ZOPT, obj.n), (L.SLM_F_UOPT, obj.n), (L.SLM_F_PNORM, S),
              (L.SLM_F_PERR, S), (L.SLM_F_OBJEVALS, S)] + ([(L.SLM_F_DNORM, S), (L.SLM_F_DERR, S)] if dual else [])
    return [summ["steps"], summ["objopt"], summ["cg_iters_total"], summ["cg_capped_updates"]] + \
           [obj.fetch(f, r) for f, r in fields]


def _object(gpu, c):
    return gpu.SparseLassoMulti(c["D"], c["S"], c["lams"], R.RIDGE, R.NONNEG)


def test_rerun_and_check_every_give_the_same_bits(gpu):
    L = gpu._lib
    c = R.case(gpu, SMALL, "shared")
    obj = _object(gpu, c)
    try:
        for dual, plan in ((True, (0, 0, 1, 8)), (False, (1, 8))):
            runs = []
            for ce in plan:
                summ = obj.run(objevals=1, check_every=ce, cg_tol=1e-13, nodualerror=0 if dual else 1, z0=c["z0"],
                               u0=c["u0"])
                runs.append(_fetch_all(L, obj, summ, dual))
            assert len(set(runs[0][0])) >= 5
            for other in runs[1:]:
                for a, b in zip(runs[0], other):
                    assert a.size > 0 and np.array_equal(a, b, equal_nan=True)
        with pytest.raises(gpu.AdmmError):  # the last run did not evaluate the dual residual
            obj.fetch(L.SLM_F_DNORM, 5)
        with pytest.raises(ValueError, match="z0"):  # z and u live on the coefficients
            obj.run(z0=np.zeros((257, R.K)))
    finally:
        obj.close()


# ---------------------------------------------------------------------------------------------- 9. weights
def test_set_weights_none_restores_the_unweighted_bits(gpu):
    L = gpu._lib
    c = R.case(gpu, SMALL, "shared")
    obj = _object(gpu, c)
    try:
        go = lambda: _fetch_all(L, obj, obj.run(objevals=1, maxiters=40, z0=c["z0"], u0=c["u0"]), True)
        plain = go()
        obj.set_weights(c["w"])
        weighted = go()
        assert not np.array_equal(plain[4], weighted[4])
        with pytest.raises(gpu.AdmmError) as err:  # a refused call changes nothing
            obj.set_weights(np.where(np.arange(65) == 3, -1.0, 1.0))
        assert err.value.code == L.E_INVALID and "weight 3" in str(err.value)
        again = go()
        obj.set_weights(None)
        restored = go()
    finally:
        obj.close()
    for a, b in zip(weighted, again):
        assert np.array_equal(a, b, equal_nan=True)
    for a, b in zip(plain, restored):
        assert np.array_equal(a, b, equal_nan=True)
    # weights handed to create are the weights of set_weights
    obj = gpu.SparseLassoMulti(c["D"], c["S"], c["lams"], R.RIDGE, R.NONNEG, c["w"])
    try:
        for a, b in zip(weighted, go()):
            assert np.array_equal(a, b, equal_nan=True)
    finally:
        obj.close()


# ---------------------------------------------------------------------------------------------- 10. the path
def test_lasso_path_grid_and_df(gpu):
    c = R.case(gpu, SMALL, "shared")
    s = c["S"][:, 0]
    g = np.abs(c["D"].T @ s.reshape(-1, 1)).reshape(-1)  # (the host's own product)
    lmax = float(g.max())
    got = gpu.lasso_path(c["D"], s, None, dict(objevals=1))
    assert got["lams"].shape == (10,) and got["lams"][0] == lmax
    np.testing.assert_allclose(got["lams"], lmax * np.logspace(0.0, -2.0, 10), rtol=1e-15)
    assert np.array_equal(got["df"], np.count_nonzero(got["zopt"], axis=0)) and got["df"][-1] > got["df"][1] >= 0
    five = gpu.lasso_path(c["D"], s, None, dict(nlambda=5, lambda_min_ratio=0.1, l1weights=c["w"]))
    live = c["w"] > 0
    assert five["lams"].shape == (5,) and five["lams"][0] == float(np.max(g[live] / c["w"][live]))
    assert abs(five["lams"][-1] / five["lams"][0] - 0.1) < 1e-15
    given = gpu.lasso_path(c["D"], s, got["lams"][[2, 6]], dict(objevals=1))
    for key in ("xopt", "zopt", "uopt"):
        assert np.array_equal(given[key], got[key][:, [2, 6]]), key
    assert list(given["df"]) == [got["df"][2], got["df"][6]]


def test_sparse_lasso_path_tester_passes(gpu):
    t = gpu.testers.sparselassopathtest(seed=0, rows=1024, cols=256, density=0.05)
    assert t["failed"] == 0 and t["zero_above_lmax"] and t["support_grows"], t["df"]
    assert t["df"][0] == 0 and t["df"][-1] > 0 and t["results"]["xsolve"] == "cg"
    assert not t["results"]["cg_capped_updates"].any()


# ---------------------------------------------------------------------------------------------- 11. refusals
def test_refusals_through_the_c_abi(gpu):
    """each returns its code with no handle, and a well-formed create succeeds right behind it; the run-time refusals"""
    L = gpu._lib
    lib = L.load()
    c = R.case(gpu, SMALL, "shared")
    csc = csc_of(c["D"])
    lam = [0.1, 0.2, 0.3]
    for name, code, part, args, kw in refusal_cases(L, c):
        rc, h = raw_create(L, *args, **kw)
        assert rc == code and not h.value and part in lib.admm_last_error().decode(), (name, rc, lib.admm_last_error())
    rc, h = raw_create(L, csc, c["S"], lam)
    assert rc == L.OK and h.value, lib.admm_last_error()
    try:
        for field, value in (("relax", 1.5), ("fast", L.FAST_STRONG), ("convtest", 1)):
            o = L.SparseLassoOptions()
            lib.admm_sparse_lasso_options_default(C.byref(o))
            setattr(o, field, value)
            assert lib.admm_sparse_lasso_run(h, C.byref(o), None, None) == L.E_UNSUPPORTED, field
            assert "sparse multi-lasso" in lib.admm_last_error().decode()
    finally:
        lib.admm_sparse_lasso_destroy(h)
