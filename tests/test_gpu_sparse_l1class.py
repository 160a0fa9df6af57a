"""The sparse linear classifier on a sparse design matrix on the device: the K lock-step runs against the
CG restatement (sparse_l1class_restated.run) per iteration and free-running, in both label modes and under both stop
rules; two chunks (bits), two runs of one object with different rho, a workgroup with several row blocks in the n-length
kernels (n > 8192) and in the row kernel (m > 8192), K = 1 against the dense object, the path, the tester, the C ABI.

Parity bound.  10x the largest relative gap between the CG restatement and the Cholesky restatement
(l1class_restated.run) over these exact problems, measured on the CPU and recorded in sparse_l1class_restated
(MEASURED_GAP): the factor q37 - q41 use for the device's summation order inside the products, and below the project's
1e-6 parity definition.  The l1 weights, the observation weights and the class costs are shared by an object: every
problem runs in two objects, fits 0 .. 5 without them and the family fit with them (on the matrix with the ones column)."""
import ctypes as C

import numpy as np
import pytest

import sparse_l1class_restated as R
from sparse_cases import csc_of
from test_gpu_sparse_lasso import _close
from test_sparse_l1class_host import raw_create, refusal_cases

pytestmark = pytest.mark.gpu

SMALL = (257, 65, 0.03)
BOUND = R.PARITY_BOUND
HIST = ("pnorm", "perr", "objevals")
KEYS = ("xopt", "zopt", "uopt", "pnorm", "perr", "dnorm", "derr", "objevals")


def _compare_fit(got, c, ref, dual, bound=BOUND):
    """column c of a multi-fit result against one reference run: steps, every history over the fit's own steps, NaN
    beyond them, the three vectors and objopt"""
    assert int(got["steps"][c]) == ref["steps"], (c, got["steps"][c], ref["steps"])
    k = ref["steps"]
    for key in HIST + (("dnorm", "derr") if dual else ()):
        _close(f"{key}[{c}]", got[key][:k, c], np.asarray(ref[key])[:k], bound)
        assert np.isnan(got[key][k:, c]).all()  # NaN past the fit's last step
    for key in ("xopt", "zopt", "uopt"):
        _close(f"{key}[{c}]", got[key][:, c], ref[key], bound)
    _close(f"objopt[{c}]", [got["objopt"][c]], [ref["objopt"]], bound)


def _device(gpu, c, cols, loop, nodualerror, starts=True, **more):
    """l1classifier_multi on the case's sparse D for the fits ``cols`` -- fits of PLAIN, or [FAMILY] alone on the matrix
    with the ones column under the family's shared members"""
    cols = list(cols)
    fits = [c["fits"][k] for k in cols]
    family = cols == [R.FAMILY]
    assert family or R.FAMILY not in cols
    E = c["ELL"] if c["ELL"].shape[1] == 1 else np.asfortranarray(c["ELL"][:, cols])
    o = dict(fits[0].options() if family else {}, **loop)
    o.update(lossfunction=[f.loss for f in fits], ridge=[f.pen.ridge for f in fits],
             nonnegative=[f.pen.nonnegative for f in fits], nodualerror=nodualerror, cg_tol=R.CG_TOL)
    if starts:
        o.update(z0=np.asfortranarray(c["z0"][:, cols]), u0=np.asfortranarray(c["u0"][:, cols]))
    o.update(more)
    return gpu.l1classifier_multi(c["Dw"] if family else c["D"], E, [f.lam for f in fits], o)


# ------------------------------------------------------------------------------------------ 1. parity per iteration
@pytest.mark.parametrize("nodualerror", (0, 1))
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_every_iteration_matches_the_restated_run(gpu, shape, mode, nodualerror):
    c = R.case(gpu, shape, mode)
    dual = not nodualerror
    got = _device(gpu, c, R.PLAIN, R.PARITY_LOOP, nodualerror)
    m, n = c["A"].shape
    assert got["xsolve"] == "cg" and got["nnz"] == c["D"].nnz and ("dnorm" in got) == dual and got["chunk"] == 10
    assert got["xopt"].shape == (n, len(R.PLAIN)) and got["zopt"].shape == (m + n, len(R.PLAIN)) == got["uopt"].shape
    assert got["pnorm"].shape == (R.PARITY_LOOP["maxiters"], len(R.PLAIN))
    for k in R.PLAIN:
        _compare_fit(got, k, R.restated_fit(gpu, shape, mode, k, R.PARITY_LOOP, nodualerror), dual)
    assert not got["cg_capped_updates"].any() and np.all(got["cg_iters_total"] >= got["steps"])
    fam = _device(gpu, c, [R.FAMILY], R.PARITY_LOOP, nodualerror)
    _compare_fit(fam, 0, R.restated_fit(gpu, shape, mode, R.FAMILY, R.PARITY_LOOP, nodualerror), dual)
    assert np.all(fam["zopt"][m:, 0] >= 0.0) and not fam["cg_capped_updates"].any()
    j = m + R.ONES_COLUMN  # l1 weight 0 and the sign constraint: z2 = max(x + u2, 0)*kappa, no threshold
    assert fam["zopt"][j, 0] >= 0.0


# ---------------------------------------------------------------------------------------------- 2. free-running
@pytest.mark.parametrize("nodualerror", (0, 1))
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_free_running_fits_stop_where_the_restated_runs_stop(gpu, shape, mode, nodualerror):
    """default tolerances, the zero start, every fit to its own stop.  Under nodualerror = 0 the hinge fit and the two
    small-lambda fits take all 1000 iterations, which costs the NumPy restatement 15 - 25 s per problem: those seven
    reference runs are the recorded ones (sparse_l1class_restated.recorded_free_dual, checked by
    test_sparse_l1class_host); under nodualerror = 1 they are computed here"""
    c = R.case(gpu, shape, mode)
    dual = not nodualerror
    if dual:
        refs = R.recorded_free_dual(shape, mode)
    else:
        refs = [R.restated_fit(gpu, shape, mode, k, None, nodualerror, free=True) for k in range(R.K)]
    steps = [r["steps"] for r in refs]
    print("reference steps", steps)
    assert len(set(steps)) >= R.FREE_DISTINCT  # on the reference alone: the fits stop at different iterations
    loop = dict(objevals=1)
    got = _device(gpu, c, R.PLAIN, loop, nodualerror, starts=False)
    for k in R.PLAIN:
        _compare_fit(got, k, refs[k], dual)
    assert not got["cg_capped_updates"].any()
    assert np.all(got["zopt"][c["A"].shape[0]:, 3] == 0.0)  # above lambda_max: the coefficient block is 0.0 exactly
    fam = _device(gpu, c, [R.FAMILY], loop, nodualerror, starts=False)
    _compare_fit(fam, 0, refs[R.FAMILY], dual)
    assert not fam["cg_capped_updates"].any()


# ---------------------------------------------------------------------------------------------- 3. chunks
def test_two_chunks_and_fits_alone_give_the_same_bits(gpu):
    """K = 12 over two chunks, fit 11 a duplicate of fit 0: bitwise equal columns, whatever the neighbours and the slot;
    the same fits run alone (K = 1) give the same bits"""
    c = R.case(gpu, SMALL, "perfit")
    kc = gpu.SparseL1Classifier.chunk()
    assert kc == 10
    cols = [k % len(R.PLAIN) for k in range(11)] + [0]
    loop = dict(objevals=1, maxiters=60)
    got = _device(gpu, c, cols, loop, 0)
    assert got["xopt"].shape == (65, 12) and got["chunk"] == kc
    steps = [int(s) for s in got["steps"]]
    print("steps", steps)
    assert min(steps) < max(steps)  # a fit stops and stays frozen while its neighbours run on
    for key in KEYS:
        for twin in (6, 11):  # fit 0 again in the first chunk and in the second
            a, b = np.ascontiguousarray(got[key][:, 0]), np.ascontiguousarray(got[key][:, twin])
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (key, twin)
    assert got["cg_iters_total"][0] == got["cg_iters_total"][11]
    for k in (0, 3, 4):
        one = _device(gpu, c, [k], loop, 0)
        s = int(one["steps"][0])
        assert s == int(got["steps"][k])
        for key in KEYS:
            rows = s if key in KEYS[3:] else None
            a, b = np.ascontiguousarray(one[key][:, 0]), np.ascontiguousarray(got[key][:rows, k])
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (key, k)
            if rows is not None:
                assert np.isnan(got[key][rows:, k]).all()


# ---------------------------------------------------------------------------------------------- 4. two runs, two rho
def _fetch_all(L, obj, summ):
    S = int(summ["steps"].max())
    fields = [(L.L1C_F_XOPT, obj.n), (L.L1C_F_ZOPT, obj.mn), (L.L1C_F_UOPT, obj.mn), (L.L1C_F_PNORM, S),
              (L.L1C_F_PERR, S), (L.L1C_F_OBJEVALS, S), (L.L1C_F_DNORM, S), (L.L1C_F_DERR, S)]
    return [summ["steps"], summ["objopt"], summ["cg_iters_total"], summ["cg_capped_updates"]] + \
           [obj.fetch(f, r) for f, r in fields]


def test_two_runs_of_one_object_with_different_rho_match_fresh_objects(gpu):
    """the shift of the x-update is 1 for every rho: nothing of a run with rho = 1 survives into the run with rho = 2.5"""
    L = gpu._lib
    c = R.case(gpu, SMALL, "perfit")
    cols = list(R.PLAIN)
    fits = [c["fits"][k] for k in cols]
    make = lambda: gpu.SparseL1Classifier(c["D"], np.asfortranarray(c["ELL"][:, cols]), [f.lam for f in fits],
                                          [f.loss for f in fits])
    z0, u0 = np.asfortranarray(c["z0"][:, cols]), np.asfortranarray(c["u0"][:, cols])
    go = lambda obj, rho: _fetch_all(L, obj, obj.run(objevals=1, maxiters=40, rho=rho, z0=z0, u0=u0))
    both = make()
    try:
        first, second = go(both, 1.0), go(both, 2.5)
        with pytest.raises(ValueError, match="z0"):  # z and u stack the rows above the coefficients
            both.run(z0=np.zeros((65, len(cols))))
    finally:
        both.close()
    for rho, kept in ((1.0, first), (2.5, second)):
        fresh = make()
        try:
            for a, b in zip(kept, go(fresh, rho)):
                assert a.size > 0 and np.array_equal(a, b, equal_nan=True)
        finally:
            fresh.close()
    assert not np.array_equal(first[4], second[4])
    ref = R.run(c["D"], R.label(c["ELL"], 2), fits[2], dict(objevals=1, maxiters=40, rho=2.5, z0=z0[:, 2].copy(),
                                                             u0=u0[:, 2].copy()))
    assert int(second[0][2]) == ref["steps"]
    _close("xopt[2] at rho = 2.5", second[4][:, 2], ref["xopt"], BOUND)
    _close("pnorm[2] at rho = 2.5", second[7][:ref["steps"], 2], ref["pnorm"], BOUND)


# ---------------------------------------------------------------------------------------------- 5. several row blocks
@pytest.mark.parametrize("shape, fits, loop", [(R.WIDE, R.WIDE_FITS, R.WIDE_LOOP), (R.TALL, R.TALL_FITS, R.TALL_LOOP)])
def test_a_workgroup_takes_several_row_blocks(gpu, shape, fits, loop):
    """60 x 8300: the n-length element and CG kernels; 8200 x 40 with objevals = 1: the row kernel
    (the CG kernels' own row-block edges, one solve at a time: test_gpu_spmm_cg.test_row_block_edges)"""
    c = R.case(gpu, shape, "shared")
    assert max(c["A"].shape) > 32 * 256 and loop["objevals"] == 1
    got = _device(gpu, c, fits, loop, 0)
    for i, k in enumerate(fits):
        _compare_fit(got, i, R.restated_fit(gpu, shape, "shared", k, loop, 0), dual=True)


# ---------------------------------------------------------------------------------------------- 6. the dense object
def test_one_fit_matches_the_dense_object(gpu):
    """ap.l1classifier on the sparse D against ap.l1classifier on D.toarray(): 10x MEASURED_GAP (the CG x-update against
    an exact one, with the device's margin) plus the dense test's own bound, 1e-6 (test_gpu_l1class.BOUND)"""
    c = R.case(gpu, SMALL, "shared")
    k = 2
    f = c["fits"][k]
    o = dict(objevals=1, maxiters=300, z0=c["z0"][:, k].copy(), u0=c["u0"][:, k].copy(), lossfunction=f.loss)
    sparse = gpu.l1classifier(c["D"], c["ELL"][:, 0], f.lam, dict(o, cg_tol=R.CG_TOL))
    dense = gpu.l1classifier(c["D"].toarray(), c["ELL"][:, 0], f.lam, o)
    assert sparse["xsolve"] == "cg" and dense["xsolve"] in ("inverse", "trsv")
    assert isinstance(sparse["cg_iters_total"], int) and sparse["cg_capped_updates"] == 0 and sparse["nnz"] == c["D"].nnz
    assert sparse["steps"] == dense["steps"]
    bound = BOUND + 1e-6
    for key in KEYS:
        _close(key, sparse[key], dense[key], bound)
    _close("objopt", [sparse["objopt"]], [dense["objopt"]], bound)


# ---------------------------------------------------------------------------------------------- 7. the path, the tester
def test_the_path_on_a_sparse_D(gpu):
    """the feature gate: on a sparse D l1classifier_path used to raise ValueError"""
    c = R.case(gpu, SMALL, "shared")
    D, ell = c["D"], c["ELL"][:, 0]
    m, n = D.shape
    got = gpu.l1classifier_path(D, ell, 10, dict(objevals=1, maxiters=300))
    lams = got["lams"]
    g = np.abs(D.T @ ell)
    assert lams.size == 10 and lams[0] == pytest.approx(0.5 * float(g.max()), rel=1e-14)
    assert lams[-1] == pytest.approx(1e-2 * lams[0], rel=1e-12) and np.all(np.diff(lams) < 0)
    assert got["xsolve"] == "cg" and got["xopt"].shape == (n, 10) and got["zopt"].shape == (m + n, 10)
    assert np.array_equal(got["df"], np.count_nonzero(got["zopt"][m:], axis=0))
    assert got["df"][-1] > got["df"][1] >= 0 and got["df"][-1] <= n - 1  # (column 7 is empty: its coefficient stays 0)
    assert np.all(got["zopt"][m + 7] == 0.0) and not got["cg_capped_updates"].any()
    given = gpu.l1classifier_path(D, ell, lams[[2, 6]], dict(objevals=1, maxiters=300))
    for key in ("xopt", "zopt", "uopt"):
        assert np.array_equal(given[key], got[key][:, [2, 6]]), key
    assert list(given["df"]) == [got["df"][2], got["df"][6]]


def test_the_tester(gpu):
    results, test = gpu.testers.sparsel1classifiertest(seed=1, rows=512, cols=96, density=0.1)
    print({k: test[k] for k in ("objopt", "zeroobj", "accuracy", "df", "steps")})
    assert test["failed"] == 0 and 0 < test["df"] < 96 and results["xsolve"] == "cg"


# ---------------------------------------------------------------------------------------------- 8. the C ABI
def test_refusals_and_setters_through_the_c_abi(gpu):
    """each create refusal returns its code with no handle, and a well-formed create succeeds right behind it; the
    run-time refusals; a refused setter changes nothing"""
    L = gpu._lib
    lib = L.load()
    c = R.case(gpu, SMALL, "perfit")
    for name, code, part, args, kw in refusal_cases(L, c):
        rc, h = raw_create(L, *args, **kw)
        assert rc == code and not h.value and part in lib.admm_last_error().decode(), (name, rc, lib.admm_last_error())
    rc, h = raw_create(L, csc_of(c["D"]), c["ELL"][:, :3], [0.1, 0.2, 0.3], xsolve=L.XSOLVE_CG)
    assert rc == L.OK and h.value, lib.admm_last_error()
    try:
        buf = np.zeros(3 * 65)
        assert lib.admm_sparse_l1class_fetch(h, L.L1C_F_XOPT, L.as_dp(buf), buf.size, None) == L.E_INVALID
        assert "before the first run" in lib.admm_last_error().decode()
        for field, value, code, needle in (("relax", 1.5, L.E_UNSUPPORTED, "sparse l1 classifier"),
                                           ("fast", L.FAST_STRONG, L.E_UNSUPPORTED, "sparse l1 classifier"),
                                           ("convtest", 1, L.E_UNSUPPORTED, "sparse l1 classifier"),
                                           ("rho", 0.0, L.E_INVALID, "rho"), ("struct_size", 4, L.E_INVALID, "struct_size")):
            o = L.SparseL1ClassOptions()
            lib.admm_sparse_l1class_options_default(C.byref(o))
            setattr(o, field, value)
            assert lib.admm_sparse_l1class_run(h, C.byref(o), None, None) == code, field
            assert needle in lib.admm_last_error().decode(), field
        w = np.ones(257)
        w[7] = -1.0
        assert lib.admm_sparse_l1class_set_cost(h, L.as_dp(w), None) == L.E_INVALID and lib.admm_last_error().decode()
        lw = np.ones(65)
        lw[2] = np.nan
        assert lib.admm_sparse_l1class_set_l1weights(h, L.as_dp(lw)) == L.E_INVALID
        assert "weight 2" in lib.admm_last_error().decode()
        o = L.SparseL1ClassOptions()
        lib.admm_sparse_l1class_options_default(C.byref(o))
        o.maxiters, o.domaxiters = 5, 1
        summ = (L.SparseL1ClassSummary * 3)()
        rt = C.c_double(0)
        L.check(lib.admm_sparse_l1class_run(h, C.byref(o), summ, C.byref(rt)))
        assert [s.steps for s in summ] == [5, 5, 5] and rt.value > 0 and all(s.xsolve == L.XSOLVE_CG for s in summ)
        assert all(s.cg_iters_total >= 5 and s.cg_capped_updates == 0 for s in summ)
        small = np.empty(3)
        assert lib.admm_sparse_l1class_fetch(h, L.L1C_F_ZOPT, L.as_dp(small), small.size, None) == L.E_CAPACITY
        assert lib.admm_sparse_l1class_fetch(h, L.L1C_F_OBJEVALS, L.as_dp(buf), buf.size, None) == L.E_INVALID
        # the measurement overwrites the iterates: what the run left can no longer be fetched
        L.check(lib.admm_sparse_l1class_fetch(h, L.L1C_F_XOPT, L.as_dp(buf), buf.size, None))
        r, e = C.c_double(0), C.c_double(0)
        L.check(lib.admm_sparse_l1class_kernel_time(h, 3, 1, C.byref(r), C.byref(e)))
        assert r.value > 0 and e.value > 0
        assert lib.admm_sparse_l1class_fetch(h, L.L1C_F_XOPT, L.as_dp(buf), buf.size, None) == L.E_INVALID
        assert "before the first run" in lib.admm_last_error().decode()
    finally:
        lib.admm_sparse_l1class_destroy(h)
