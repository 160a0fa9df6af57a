"""The multi-fit robust regression on a sparse design matrix on the device: the K lock-step runs against
the oracle per fit in the three modes, the dual residual against the oracle's default lad / huberfit, the single-fit entry
points, two chunks, a workgroup with several row blocks, rank-deficient matrices against the restatement, freezing, the
reported iteration cap, reruns, weights, refusals.

Parity bound.  The largest relative gap between the NumPy restatement (cg_tol = 1e-13) and the oracle over these exact
problems, fits, both stop rules and every field (dnorm / derr included) is 2.585e-09, measured by test_sparse_reg_host
(the epsilon-insensitive fit on 600x120, per-fit S, nodualerror = 0); the bound here is 10x the recorded 2.6e-9 =
2.6e-8 -- the factor covers the device's summation order inside the products -- and below the project's 1e-6 parity
definition.  The oracle has the plain LAD and Huber losses only: the other members of the family are compared against
the oracle's loop with the restated prox (loss_restated.run), as test_gpu_reg_multi does.  The runs with
nodualerror = 0 stop at sparse_reg_restated.DUAL_MAXITERS iterations at the latest (the oracle's as well)."""
import ctypes as C

import numpy as np
import pytest

import sparse_reg_restated as R
from sparse_cases import csc_of
from sparse_cases import problem as lasso_problem
from test_sparse_reg_host import raw_create, refusal_cases

pytestmark = pytest.mark.gpu

SMALL = (257, 65, 0.03)
BOUND = R.PARITY_BOUND


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
    for key in ("pnorm", "perr", "objevals") + (("dnorm", "derr") if dual else ()):
        _close(f"{key}[{c}]", got[key][:k, c], np.asarray(ref[key])[:k], BOUND)
        assert np.isnan(got[key][k:, c]).all()  # NaN past the fit's last step
    for key in ("xopt", "zopt", "uopt"):
        _close(f"{key}[{c}]", got[key][:, c], ref[key], BOUND)
    _close(f"objopt[{c}]", [got["objopt"][c]], [ref["objopt"]], BOUND)


def _multi(gpu, c, nodualerror, cols=None, **more):
    """robustfit_multi on the case's sparse D for the fits `cols` (default all seven) with their own starts"""
    cols = list(range(len(R.FITS))) if cols is None else list(cols)
    S = c["S"] if c["S"].shape[1] == 1 else np.asfortranarray(c["S"][:, cols])
    o = dict(R.loop_options(nodualerror), cg_tol=1e-13, z0=np.asfortranarray(c["z0"][:, cols]),
             u0=np.asfortranarray(c["u0"][:, cols]))
    if c["w"] is not None:
        o["weights"] = c["w"]
    o.update(more)
    return gpu.robustfit_multi(c["D"], S, [R.FITS[k] for k in cols], o)


# ---------------------------------------------------------------------------------------------- 1. parity per fit
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_fits_match_the_oracle_per_fit(gpu, shape, mode):
    c = R.case(gpu, shape, mode)
    refs = [R.oracle_fit(gpu, shape, mode, k, 1) for k in range(len(R.FITS))]
    assert len({r["steps"] for r in refs}) >= 5  # the fits stop at different iterations: the test of freezing
    got = _multi(gpu, c, 1)
    assert got["xsolve"] == "cg" and got["nnz"] == c["D"].nnz and "fallback" not in got and "dnorm" not in got
    assert list(got["steps"]) == [r["steps"] for r in refs]
    assert got["pnorm"].shape == (max(r["steps"] for r in refs), len(R.FITS))
    for k, ref in enumerate(refs):
        _compare_fit(got, k, ref, dual=False)
    assert not got["cg_capped_updates"].any() and np.all(got["cg_iters_total"] >= got["steps"])


# ---------------------------------------------------------------------------------------------- 2. the dual residual
def test_dual_residual_matches_the_default_lad_and_huberfit(gpu):
    """nodualerror = 0: fits 0 and 4 are the oracle's own lad / huberfit under their default stop rule"""
    c = R.case(gpu, SMALL, "shared")
    refs = [R.oracle_fit(gpu, SMALL, "shared", k, 0) for k in range(len(R.FITS))]
    assert refs[4]["steps"] < R.DUAL_MAXITERS and refs[5]["steps"] < R.DUAL_MAXITERS  # both residuals stop them
    assert all(r["steps"] > R.oracle_fit(gpu, SMALL, "shared", k, 1)["steps"] for k, r in enumerate(refs))
    got = _multi(gpu, c, 0)
    assert list(got["steps"]) == [r["steps"] for r in refs]
    for k, ref in enumerate(refs):
        _compare_fit(got, k, ref, dual=True)


def test_single_fit_entry_points_are_the_one_fit_object(gpu):
    """lad(<sparse>), huberfit(<sparse>) and quantilereg(<sparse>, tau) pass the reference's default nodualerror = 0 and
    equal column 0 of the K = 1 object bit for bit"""
    c = R.case(gpu, SMALL, "shared")
    s = c["S"][:, 0]
    calls = ((0, lambda o: gpu.lad(c["D"], s, o)), (4, lambda o: gpu.huberfit(c["D"], s, o)),
             (1, lambda o: gpu.quantilereg(c["D"], s, R.FITS[1]["tau"], o)))
    for k, call in calls:
        one = call(dict(objevals=1, cg_tol=1e-13, maxiters=60, z0=c["z0"][:, k], u0=c["u0"][:, k]))
        multi = _multi(gpu, c, 0, [k], maxiters=60)
        assert one["steps"] == int(multi["steps"][0]) and one["xsolve"] == "cg" and one["nnz"] == c["D"].nnz
        assert "xvals" not in one and one["xopt"].shape == (65,) and "fallback" not in one and "chunk" not in one
        for key in ("xopt", "zopt", "uopt", "pnorm", "perr", "dnorm", "derr", "objevals"):
            assert np.array_equal(one[key], multi[key][:, 0]), key
        assert one["objopt"] == multi["objopt"][0] and one["cg_iters_total"] == int(multi["cg_iters_total"][0])
        assert one["cg_capped_updates"] == 0
        if k == 4:  # the Huber fit stops on both residuals inside these 60 iterations, as the oracle's huberfit does
            assert one["steps"] == R.oracle_fit(gpu, SMALL, "shared", 4, 0)["steps"] < 60


# ---------------------------------------------------------------------------------------------- 3. chunks
def test_two_chunks(gpu):
    """K = Kc + 1 with the last fit a duplicate of fit 0: bitwise equal columns; K = Kc and K = 1 give the same bits"""
    c = R.case(gpu, SMALL, "shared")
    kc = gpu.SparseRegMulti.chunk()
    assert kc == 10
    cols = [k % len(R.FITS) for k in range(kc)] + [0]
    got = _multi(gpu, c, 1, cols)
    assert got["xopt"].shape == (65, kc + 1) and got["chunk"] == kc
    for k in (0, kc):
        _compare_fit(got, k, R.oracle_fit(gpu, SMALL, "shared", 0, 1), dual=False)
    keys = ("xopt", "zopt", "uopt", "pnorm", "perr", "objevals")
    for key in keys:
        assert np.array_equal(got[key][:, kc], got[key][:, 0], equal_nan=True), key
        assert np.array_equal(got[key][:, 7], got[key][:, 0], equal_nan=True), key
    ten = _multi(gpu, c, 1, cols[:kc])
    one = _multi(gpu, c, 1, [0])
    S1 = int(one["steps"][0])
    for key in keys:
        assert np.array_equal(ten[key], got[key][:, :kc], equal_nan=True), key
        rows = S1 if key in ("pnorm", "perr", "objevals") else None
        assert np.array_equal(one[key][:, 0], got[key][:rows, 0]), key
    assert np.array_equal(ten["cg_iters_total"], got["cg_iters_total"][:kc])


# ---------------------------------------------------------------------------------------------- 4. several row blocks
def test_a_workgroup_takes_several_row_blocks(gpu):
    """(the CG kernels' own row-block edges, one solve at a time: test_gpu_spmm_cg.test_row_block_edges)"""
    c = R.tall_case(gpu)
    assert c["A"].shape[0] > 32 * 256
    got = _multi(gpu, c, 1, R.TALL_FITS, maxiters=R.TALL_MAXITERS)
    for i, k in enumerate(R.TALL_FITS):
        _compare_fit(got, i, R.tall_oracle(gpu, k), dual=False)


# ---------------------------------------------------------------------------------------------- 5. rank deficiency
def _against_the_restatement(gpu, A, cols, **more):
    c = R.case(gpu, A.shape + (0.0,), "shared", A=np.asfortranarray(A))
    got = _multi(gpu, c, 1, cols, **more)
    for i, k in enumerate(cols):
        _compare_fit(got, i, R.restated_fit(c, k, 1, **more), dual=False)
    assert not got["cg_capped_updates"].any()
    return got


def test_an_empty_column_keeps_x_exactly_zero(gpu):
    A = R.matrix(gpu, *SMALL, full_rank=False)
    assert not A[:, 7].any()
    got = _against_the_restatement(gpu, A, [0, 1, 4])
    assert np.all(got["xopt"][7, :] == 0.0)


def test_a_duplicated_column_gets_equal_coefficients(gpu):
    A = R.matrix(gpu, *SMALL, full_rank=False)
    A[:, 7] = A[:, 9]
    assert np.linalg.matrix_rank(A) == 64
    got = _against_the_restatement(gpu, A, [1, 5])
    # two equal rows of D' see the same products in the same order in every solve
    assert np.array_equal(got["xopt"][7, :], got["xopt"][9, :]) and np.all(got["xopt"][7, :] != 0.0)


def test_more_columns_than_rows(gpu):
    """80 x 200: the dense object refuses m < n; the minimum-norm x-update runs it"""
    A = lasso_problem(gpu, 80, 200, 0.10, seed=3)["A"]
    got = _against_the_restatement(gpu, A, [0, 3, 4], maxiters=60)
    assert got["xopt"].shape == (200, 3) and np.all(got["xopt"][7, :] == 0.0)


# ---------------------------------------------------------------------------------------------- 6. freezing
def test_a_stopped_fit_is_frozen(gpu):
    """the Huber fit stops after a few iterations; the others run on for a hundred more: its x, z, u are those of its
    own run"""
    c = R.case(gpu, SMALL, "shared")
    got = _multi(gpu, c, 1)
    alone = _multi(gpu, c, 1, [4])
    assert int(alone["steps"][0]) == int(got["steps"][4]) < int(got["steps"].max()) - 50
    for key in ("xopt", "zopt", "uopt"):
        assert np.array_equal(alone[key][:, 0], got[key][:, 4]), key
    S4 = int(alone["steps"][0])
    for key in ("pnorm", "perr", "objevals"):
        assert np.array_equal(alone[key][:, 0], got[key][:S4, 4]), key


# ---------------------------------------------------------------------------------------------- 7. the cap
def test_the_iteration_cap_is_reported(gpu):
    c = R.case(gpu, (600, 120, 0.05), "shared")
    got = _multi(gpu, c, 1, maxiters=30, cg_maxit=2)
    assert np.all(got["steps"] >= 1) and np.isfinite(got["xopt"]).all()
    assert got["cg_capped_updates"].shape == (len(R.FITS),) and np.all(got["cg_capped_updates"] > 0)
    assert np.all(got["cg_iters_total"] <= 2 * got["steps"])


# ---------------------------------------------------------------------------------------------- 8. same bits
def _fetch_all(L, obj, summ, dual):
    S = int(summ["steps"].max())
    fields = [(L.SRG_F_XOPT, obj.n), (L.SRG_F_ZOPT, obj.m), (L.SRG_F_UOPT, obj.m), (L.SRG_F_PNORM, S),
              (L.SRG_F_PERR, S), (L.SRG_F_OBJEVALS, S)] + ([(L.SRG_F_DNORM, S), (L.SRG_F_DERR, S)] if dual else [])
    return [summ["steps"], summ["objopt"], summ["cg_iters_total"], summ["cg_capped_updates"]] + \
           [obj.fetch(f, r) for f, r in fields]


def _object(gpu, c):
    fl = [R.loss_of(f) for f in R.FITS]
    return gpu.SparseRegMulti(c["D"], c["S"], [0 if f.kind == "lad" else 1 for f in fl], [f.a for f in fl],
                              [f.b for f in fl], [f.eps for f in fl], [f.delta for f in fl])


def test_rerun_and_check_every_give_the_same_bits(gpu):
    L = gpu._lib
    c = R.case(gpu, SMALL, "shared")
    obj = _object(gpu, c)
    try:
        for dual, plan, more in ((False, (0, 0, 1, 8), {}), (True, (1, 8), dict(maxiters=40))):
            runs = []
            for ce in plan:
                summ = obj.run(objevals=1, check_every=ce, cg_tol=1e-13, nodualerror=0 if dual else 1, z0=c["z0"],
                               u0=c["u0"], **more)
                runs.append(_fetch_all(L, obj, summ, dual))
            assert dual or len(set(runs[0][0])) >= 5
            for other in runs[1:]:
                for a, b in zip(runs[0], other):
                    assert a.size > 0 and np.array_equal(a, b, equal_nan=True)
        with pytest.raises(gpu.AdmmError):  # the last run evaluated the dual residual; one without it has no dnorm
            obj.run(objevals=1, maxiters=5)
            obj.fetch(L.SRG_F_DNORM, 5)
    finally:
        obj.close()


# ---------------------------------------------------------------------------------------------- 9. weights
def test_set_weights_none_restores_the_unweighted_bits(gpu):
    L = gpu._lib
    c = R.case(gpu, SMALL, "weighted")
    obj = _object(gpu, c)
    try:
        go = lambda: _fetch_all(L, obj, obj.run(objevals=1, maxiters=40, z0=c["z0"], u0=c["u0"]), False)
        plain = go()
        obj.set_weights(c["w"])
        weighted = go()
        assert not np.array_equal(plain[4], weighted[4])
        with pytest.raises(gpu.AdmmError) as err:  # a refused call changes nothing
            obj.set_weights(np.where(np.arange(257) == 3, -1.0, 1.0))
        assert err.value.code == L.E_INVALID and "weight 3" in str(err.value)
        again = go()
        obj.set_weights(None)
        restored = go()
    finally:
        obj.close()
    for a, b, d in zip(weighted, again, restored):
        assert np.array_equal(a, b, equal_nan=True)
    for a, b in zip(plain, restored):
        assert np.array_equal(a, b, equal_nan=True)


# ---------------------------------------------------------------------------------------------- 10. refusals
def test_refusals_through_the_c_abi(gpu):
    """each returns its code with no handle, and a well-formed create succeeds right behind it; the run-time refusals"""
    L = gpu._lib
    lib = L.load()
    c = R.case(gpu, SMALL, "shared")
    csc = csc_of(c["D"])
    for name, code, part, args, kw in refusal_cases(L, c):
        rc, h = raw_create(L, *args, **kw)
        assert rc == code and not h.value and part in lib.admm_last_error().decode(), (name, rc, lib.admm_last_error())
        rc, h = raw_create(L, csc, c["S"], 3)
        assert rc == L.OK and h.value, (name, lib.admm_last_error())
        lib.admm_sparse_reg_destroy(h)
    rc, h = raw_create(L, csc, c["S"], 3)
    assert rc == L.OK
    try:
        for field, value in (("relax", 1.5), ("fast", L.FAST_STRONG), ("convtest", 1)):
            o = L.SparseRegOptions()
            lib.admm_sparse_reg_options_default(C.byref(o))
            setattr(o, field, value)
            assert lib.admm_sparse_reg_run(h, C.byref(o), None, None) == L.E_UNSUPPORTED, field
    finally:
        lib.admm_sparse_reg_destroy(h)


def test_no_limit_on_n_and_no_fallback(gpu):
    A = lasso_problem(gpu, 700, 500, 0.02, seed=3)["A"]
    import scipy.sparse as sp
    s = A @ np.random.default_rng(5).standard_normal(500) + 0.1 * np.random.default_rng(6).standard_normal(700)
    got = gpu.quantilereg_multi(sp.csr_matrix(A), s, [0.25, 0.75], dict(maxiters=10, objevals=1))
    assert "fallback" not in got and got["xsolve"] == "cg" and got["xopt"].shape == (500, 2)
    assert list(got["taus"]) == [0.25, 0.75] and np.isfinite(got["xopt"]).all() and np.all(got["xopt"][7, :] == 0.0)


def test_sparse_quantile_tester_passes(gpu):
    """the pass property of quantileregmultitest on a sparse D with a dense intercept column: for every tau,
    #(z < 0) <= tau*m <= #(z <= 0) on that fit's final z"""
    t = gpu.testers.sparsequantileregtest(seed=0, rows=1024, cols=64, density=0.05)
    assert t["failed"] == 0 and t["slack"] == [0.0] * 5, t["slack"]
    assert t["results"]["xsolve"] == "cg" and "fallback" not in t["results"] and t["D"].shape == (1024, 64)
    assert not t["results"]["cg_capped_updates"].any()
