"""Group lasso on the device: the block soft threshold against long double, singleton groups against plain lasso, full
runs of every iteration form against the restatement (tests/grouplasso_restated.py) at the project's per-iteration
tolerance 1e-7, the launch count of the element update, the setter's edges, the tester and the MEX gateway."""
import ctypes as C

import numpy as np
import pytest

import grouplasso_restated as R

pytestmark = pytest.mark.gpu

# a singleton; runs that end on (1 + 127 = 128), before and past 128-element boundaries; 200 and 300 are larger than the
# plan's starting budget of one 128-element tile (loop_kernels.h: kGroupTile), so each has a workgroup of its own that
# walks it in several chunks -- no further size is needed for that case
SIZES = [1, 127, 1, 200, 3, 300, 68]
PLAIN = ("xvals", "zvals", "uvals", "pnorm", "dnorm", "perr", "derr", "objevals")
STRONG = PLAIN + ("vvals", "uhatvals", "avals")
WEAK = ("xvals", "zvals", "uvals", "vvals", "uhatvals", "objevals", "avals", "dvals", "restarted")  # (admm.m records no norms there)


def _err(name, got, ref, tol=1e-7):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert not np.isnan(got).any() and not np.isnan(ref).any(), f"{name}: NaN"
    err = float(np.max(np.abs(got - ref)) / max(1e-300, np.max(np.abs(ref))))
    print(f"{name}: relative error {err:.3e} (bound {tol:g})")
    assert err < tol, f"{name}: relative error {err:.3e} >= {tol:g}"


def _same_run(got, ref, steps=None, hist=PLAIN, tol=1e-7):
    """every history of the case (a missing one is a failure), the final iterates, the objective and the step count"""
    assert int(got["steps"]) == int(ref["steps"]), (got["steps"], ref["steps"])
    if steps is not None:
        assert int(got["steps"]) == steps
    for key in hist:
        assert key in got and key in ref, key
        _err(key, got[key], ref[key], tol)
    for key in ("xopt", "zopt", "uopt"):
        _err(key, got[key], ref[key], tol)
    _err("objopt", [got["objopt"]], [ref["objopt"]], tol)


def _problem(gpu, rows, cols, sizes, seed, weights=None, active=(1, 3)):
    """lassotest's D (unit columns) with a group-sparse truth; lambda = a tenth of the smallest one that zeroes every group"""
    assert sum(sizes) == cols
    D = gpu.synth.lasso_problem(seed, rows, cols)["D"]
    rng = np.random.default_rng(seed + 100)
    off = R.offsets(sizes)
    xt = np.zeros(cols)
    for g in active:
        if g < len(sizes):
            xt[off[g]:off[g + 1]] = rng.standard_normal(sizes[g])
    s = D @ xt + np.sqrt(0.001) * rng.standard_normal(rows)
    w = R.weights_of(sizes, weights)
    g0 = D.T @ s
    lam = 0.1 * max(float(np.linalg.norm(g0[off[g]:off[g + 1]])) / max(w[g], 1e-300) for g in range(len(sizes)))
    return dict(D=D, s=s, lam=lam, sizes=list(sizes), weights=weights)


def _run_both(gpu, p, opts, ref_opts=None):
    o = dict(opts)
    if p["weights"] is not None:
        o["groupweights"] = p["weights"]
    got = gpu.grouplasso(p["D"], p["s"], p["lam"], p["sizes"], o)
    ro = dict(opts if ref_opts is None else ref_opts)
    for k in ("xsolve", "record_history"):
        ro.pop(k, None)
    ref = R.run(p["D"], p["s"], p["lam"], p["sizes"], ro, weights=p["weights"])
    return got, ref


# ------------------------------------------------------------------------------------------- the shrinkage alone
def _device_shrink(gpu, v, sizes, t, weights=None):
    lib = gpu._lib.load()
    v = np.ascontiguousarray(v, dtype=np.float64)
    out = np.full(v.size, np.nan)
    sz = np.ascontiguousarray(sizes, dtype=np.int64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    gpu._lib.check(lib.admm_op_group_soft_threshold(gpu._lib.as_dp(v), v.size, sz.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    sz.size, None if w is None else gpu._lib.as_dp(w), float(t),
                                                    gpu._lib.as_dp(out)))
    return out


def _check_shrink(v, out, sizes, t, weights=None):
    """per element |out_i - exact_i| <= (p_g + 8)*eps*|v_i|: a p_g-term sum of squares in any order, the square root,
    the division, the subtraction and the product; near ||v_g|| = t both branches lie within it"""
    exact = R.shrink(v, sizes, t, weights, dtype=np.longdouble)
    off = R.offsets(sizes)
    worst = 0.0
    for g, p in enumerate(sizes):
        sl = slice(off[g], off[g + 1])
        bound = (p + 8) * R.EPS * np.abs(v[sl]).astype(np.longdouble)
        d = np.abs(out[sl].astype(np.longdouble) - exact[sl])
        assert np.all(d <= bound), (g, p, float(np.max(d - bound)))
        nz = bound > 0
        if nz.any():
            worst = max(worst, float(np.max(d[nz] / bound[nz])))
    print(f"t = {t:g}: worst |out - exact| / bound = {worst:.3f}")
    return exact


@pytest.mark.parametrize("case", ["t=0", "t=1e-12", "median", "above", "zero-group"])
def test_shrinkage_against_long_double(gpu, case):
    rng = np.random.default_rng(11)
    v = rng.standard_normal(700)
    off = R.offsets(SIZES)
    if case == "zero-group":
        v[off[3]:off[4]] = 0.0
    norms = np.array([np.linalg.norm(v[off[g]:off[g + 1]]) for g in range(len(SIZES))])
    t = {"t=0": 0.0, "t=1e-12": 1e-12, "median": float(np.median(norms)), "above": 2.0 * float(norms.max()),
         "zero-group": float(np.median(norms))}[case]
    out = _device_shrink(gpu, v, SIZES, t)
    assert np.isfinite(out).all()
    exact = _check_shrink(v, out, SIZES, t)
    if case == "t=0":
        assert np.array_equal(out, v)  # bit for bit
    if case == "above":
        assert np.array_equal(out, np.zeros(700))
    if case == "median":
        assert np.any(exact == 0) and np.any(exact != 0)
    if case == "zero-group":
        assert np.array_equal(out[off[3]:off[4]], np.zeros(200))


def test_shrinkage_weights_and_a_raised_budget(gpu):
    """2100 groups of 65 make 2100 workgroups at the starting budget, more than the block partials hold: the budget
    doubles to 256 and a workgroup takes three groups = 195 elements = two chunks, with a group across the chunk
    boundary; a tail of singletons and one group of 1000 behind them; weights, a zero weight among them"""
    sizes = [65] * 2100 + [1] * 37 + [1000]
    rng = np.random.default_rng(12)
    w = rng.uniform(0.5, 2.0, len(sizes))
    w[5] = 0.0
    v = rng.standard_normal(sum(sizes))
    t = 7.0  # E||v_g|| is about 8 for p = 65
    out = _device_shrink(gpu, v, sizes, t, w)
    exact = _check_shrink(v, out, sizes, t, w)
    assert np.any(exact == 0) and np.any(exact != 0)
    assert np.array_equal(out[5 * 65:6 * 65], v[5 * 65:6 * 65])  # weight 0: the group passes unchanged


def test_shrinkage_refuses_bad_groups(gpu):
    L = gpu._lib
    v = np.ones(8)
    for sizes, w, code in (([3, 4], None, L.E_INVALID), ([3, 0, 5], None, L.E_INVALID), ([3, 5], [1.0, -1.0], L.E_INVALID),
                           ([3, 5], [1.0, float("nan")], L.E_INVALID)):
        with pytest.raises(gpu.AdmmError) as ei:
            _device_shrink(gpu, v, sizes, 0.5, w)
        assert ei.value.code == code


# ------------------------------------------------------------------------------------------- singleton groups
def test_singleton_groups_are_plain_lasso(gpu):
    """p_g = 1, w_g = 1: ||v_g|| = |v_i| and the block soft threshold is the soft threshold, up to its rounding"""
    p = gpu.synth.lasso_problem(0, 256, 64)
    o = dict(objevals=1)
    got = gpu.grouplasso(p["D"], p["s"], p["lam"], [1] * 64, o)
    ref = gpu.lasso(p["D"], p["s"], p["lam"], o)
    assert got["engine_info"]["ngroups"] == 64 and ref["engine_info"]["ngroups"] == 0
    _same_run(got, ref, tol=1e-12)


# ------------------------------------------------------------------------------------------- full runs
@pytest.fixture(scope="module")
def tall(gpu):
    return _problem(gpu, 1024, 700, SIZES, 3)


@pytest.fixture(scope="module")
def wide(gpu):
    """512 x 700 as the issue writes it (fewer rows than columns: the engine's fat-lasso x-update)"""
    return _problem(gpu, 512, 700, SIZES, 4)


@pytest.mark.parametrize("which", ["tall", "wide"])
def test_run_to_the_stop(gpu, tall, wide, which):
    p = tall if which == "tall" else wide
    got, ref = _run_both(gpu, p, dict(objevals=1))
    assert 5 <= ref["steps"] < 1000
    off = R.offsets(SIZES)
    zero = [not np.any(ref["zopt"][off[g]:off[g + 1]]) for g in range(len(SIZES))]
    assert any(zero) and not all(zero)  # the penalty is at work: on a build that ignores the groups this run differs
    _same_run(got, ref)


@pytest.mark.parametrize("which", ["tall", "wide"])
def test_forced_30_iterations(gpu, tall, wide, which):
    p = tall if which == "tall" else wide
    got, ref = _run_both(gpu, p, dict(objevals=1, maxiters=30, domaxiters=1))
    _same_run(got, ref, steps=30)


def test_fat_48_x_300(gpu):
    p = _problem(gpu, 48, 300, [100, 100, 1, 99], 5, active=(0, 2))
    got, ref = _run_both(gpu, p, dict(objevals=1))
    _same_run(got, ref)


def test_one_group_of_n(gpu):
    """sizes = [n]: one workgroup; z = v*(1 - t/||v||)"""
    p = _problem(gpu, 256, 64, [64], 6, active=(0,))
    got, ref = _run_both(gpu, p, dict(objevals=1))
    assert np.any(ref["zopt"])
    _same_run(got, ref)


@pytest.mark.parametrize("opts,hist", [
    (dict(), PLAIN), (dict(relax=1.6), PLAIN),
    (dict(fast=1, fasttype="strong"), STRONG), (dict(fast=1, fasttype="weak"), WEAK),
    (dict(xsolve="trsv"), PLAIN), (dict(xsolve="inverse"), PLAIN),
], ids=["sqrt-weights", "relax", "strong", "weak", "trsv", "inverse"])
def test_variants_with_sqrt_weights(gpu, opts, hist):
    """non-unit weights sqrt(p_g) throughout, on 1024 x 700"""
    w = np.sqrt(np.asarray(SIZES, dtype=np.float64))
    p = _problem(gpu, 1024, 700, SIZES, 7, weights=w)
    got, ref = _run_both(gpu, p, dict(opts, objevals=1, maxiters=40))
    if "xsolve" in opts:
        assert got["engine_info"]["xsolve_used"] == opts["xsolve"]
    _same_run(got, ref, hist=hist)


def test_record_history_off(gpu, tall):
    got, ref = _run_both(gpu, tall, dict(objevals=1, record_history=0))
    assert "xvals" not in got
    _same_run(got, ref, hist=("pnorm", "dnorm", "perr", "derr", "objevals"))


def test_warm_start(gpu, tall):
    rng = np.random.default_rng(8)
    o = dict(objevals=1, x0=rng.standard_normal(700), z0=rng.standard_normal(700), u0=0.1 * rng.standard_normal(700))
    got, ref = _run_both(gpu, tall, o)
    _same_run(got, ref)


@pytest.mark.parametrize("form", ["inverse", "one"])
def test_partial_rows_of_the_x_solve(gpu, form, monkeypatch):
    """n = 1600 >= 1536: the x-solve leaves its partial rows to the element update -- the packed lower-triangle product
    (N-part and T-part rows, deferred finalize) and the one-block triangular solves (rows from the diagonal tile on).
    Groups cross the 128-element tiles of those rows; 300, 400 and 500 span several of them.  12 forced iterations of
    plain and of strong fast ADMM"""
    sizes = SIZES + [500, 400]
    p = _problem(gpu, 2000, 1600, sizes, 9, active=(1, 3, 7))
    if form == "one":
        monkeypatch.setenv("ADMM_TRSV_FORM", "one")
    xs = "inverse" if form == "inverse" else "trsv"
    for extra, hist in ((dict(), PLAIN), (dict(fast=1, fasttype="strong"), STRONG)):
        got, ref = _run_both(gpu, p, dict(extra, objevals=1, maxiters=12, domaxiters=1, xsolve=xs))
        info = got["engine_info"]
        assert info["xsolve_used"] == xs and (form != "one" or info["trsv_blocks"] == 1)
        _same_run(got, ref, steps=12, hist=hist)


# ------------------------------------------------------------------------------------------- launches, setter
def _engine_run(gpu, eng, n, **kw):
    L = gpu._lib
    eng.run(maxiters=30, domaxiters=1, objevals=1, **kw)
    return {k: eng.fetch(f, n) for k, f in (("x", L.F_XOPT), ("z", L.F_ZOPT), ("u", L.F_UOPT))} | \
        {k: eng.fetch(f, 30) for k, f in (("pnorm", L.F_PNORM), ("dnorm", L.F_DNORM), ("obj", L.F_OBJEVALS))}


def test_one_launch_and_setter_edges(gpu, tall):
    """the forced 30-iteration run: the element update is one launch group per iteration with and without groups;
    set_groups(None) afterwards makes the same engine reproduce plain lasso bit for bit"""
    L = gpu._lib
    D, s, lam = tall["D"], tall["s"], tall["lam"]
    eng = gpu.Engine(L.PROB_LASSO, D=D, s=s, lam=lam)
    try:
        eng.set_profiling([L.K_PROX, L.K_FINALIZE, L.K_XSOLVE])
        _engine_run(gpu, eng, 700)  # (an engine's first objevals run calibrates the objective's form: other launches)
        plain = _engine_run(gpu, eng, 700)
        counts = [eng.kernel_time(k)[1] for k in (L.K_PROX, L.K_FINALIZE, L.K_XSOLVE)]
        assert counts[0] == 30 and eng.info()["ngroups"] == 0
        eng.set_groups(SIZES)
        assert eng.info()["ngroups"] == len(SIZES)
        grouped = _engine_run(gpu, eng, 700)
        assert [eng.kernel_time(k)[1] for k in (L.K_PROX, L.K_FINALIZE, L.K_XSOLVE)] == counts
        ref = R.run(D, s, lam, SIZES, dict(objevals=1, maxiters=30, domaxiters=1))
        _err("grouped zopt", grouped["z"], ref["zopt"])
        _err("grouped objevals", grouped["obj"], ref["objevals"])
        assert not np.array_equal(grouped["z"], plain["z"])
        again = _engine_run(gpu, eng, 700)
        for k in grouped:
            assert np.array_equal(again[k], grouped[k]), k  # fixed summation order: bitwise reproducible
        for bad in ([1, 2], [700, 0], [-1, 701]):
            with pytest.raises(gpu.AdmmError) as ei:
                eng.set_groups(bad)
            assert ei.value.code == L.E_INVALID
        with pytest.raises(gpu.AdmmError) as ei:
            eng.set_groups(SIZES, [1.0] * 6 + [-1.0])
        assert ei.value.code == L.E_INVALID and eng.info()["ngroups"] == len(SIZES)  # a refused call changes nothing
        eng.set_groups(None)
        assert eng.info()["ngroups"] == 0
        back = _engine_run(gpu, eng, 700)
        for k in plain:
            assert np.array_equal(back[k], plain[k]), k
    finally:
        eng.close()


def test_set_groups_on_an_svm_engine_is_unsupported(gpu):
    L = gpu._lib
    p = gpu.synth.svm_problem(0)
    eng = gpu.Engine(L.PROB_LINEARSVM, D=p["D"], ell=p["ell"], Cval=p["C"])
    try:
        with pytest.raises(gpu.AdmmError) as ei:
            eng.set_groups([p["D"].shape[0]])
        assert ei.value.code == L.E_UNSUPPORTED
    finally:
        eng.close()


def test_a_zming_callback_wins_over_the_groups(gpu):
    """the caller's z-update replaces the grouped one as it replaces the l1 prox"""
    import torch
    p = gpu.synth.lasso_problem(2, 256, 64)
    args = dict(D=p["D"], s=p["s"], groups=[16] * 4)
    args["lambda"] = p["lam"]
    gx, _, _ = gpu.getproxops("LASSO", args)
    lam = p["lam"]
    zmin = lambda x, _z, u, rho: torch.sign(x + u) * torch.clamp(torch.abs(x + u) - lam / rho, min=0.0)
    got = gpu.admm(gx, zmin, dict(A=1, At=1, m=64, nA=64, nB=64, B=-1, c=0))
    ref = gpu.lasso(p["D"], p["s"], p["lam"], {})
    assert int(got["steps"]) == int(ref["steps"])
    for key in ("xvals", "zvals", "uvals", "pnorm", "dnorm", "xopt", "zopt"):
        _err(key, got[key], ref[key], 1e-12)


# ------------------------------------------------------------------------------------------- tester, gateway
@pytest.mark.parametrize("seed", [0, 1])
def test_grouplassotest(gpu, seed):
    results, test = gpu.testers.grouplassotest(seed=seed)
    print(f"objopt {test['objopt']:.6f} < testobj {test['testobj']:.6f}, {test['steps']} steps")
    assert test["failed"] == 0
    off = R.offsets(test["groups"])
    zero = [not np.any(results["zopt"][off[g]:off[g + 1]]) for g in range(len(test["groups"]))]
    assert any(zero)  # group-sparse: whole groups are exactly zero


def test_mex_gateway_groups(gpu, tmp_path_factory):
    """args.groups / args.groupweights reach the setter through the binding layer with no change to the gateway"""
    from mexharness import Harness, build
    mex = Harness(build(tmp_path_factory.mktemp("mexgroups")))
    sizes = [1, 20, 7, 36]
    w = np.sqrt(np.asarray(sizes, dtype=np.float64))
    p = _problem(gpu, 256, 64, sizes, 10, weights=w, active=(1,))
    D, s, lam = p["D"], p["s"], p["lam"]
    args = dict(D=D, s=s, m=256, n=64, parallel=0, rho=1.0, groups=np.asarray(sizes, dtype=np.float64), groupweights=w)
    args["lambda"] = lam
    options = dict(objevals=1, A=1, At=1, m=64, nA=64, nB=64, B=-1, c=0, parallel="none")
    got = mex.call("solve", "lasso", args, options, dict(objnative=1, s=s))
    ref = gpu.grouplasso(D, s, lam, sizes, dict(objevals=1, groupweights=w))
    assert int(got["steps"]) == int(ref["steps"])
    for key in ("xopt", "zopt", "zvals", "objevals"):
        _err(key, got[key], ref[key], 1e-12)
    plain = gpu.lasso(D, s, lam, dict(objevals=1))
    assert not np.allclose(plain["zopt"], ref["zopt"], rtol=1e-6, atol=1e-9)
    args["groups"] = np.asarray([1.0, 20.0, 7.0, 35.0])
    from mexharness import MexError
    with pytest.raises(MexError):
        mex.call("solve", "lasso", args, options, dict(objnative=1, s=s))
