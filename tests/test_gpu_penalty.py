"""The lasso's penalty family on the device: the prox operator against long double, full runs of every
iteration form against the restatement (tests/penalty_restated.py) at the project's per-iteration tolerance 1e-7, the
launch counts, reproducibility, the setter's edges, the tester and the MEX gateway.  tests/test_penalty_host.py checks on
the CPU that the fixtures used here have solutions the penalty has shaped."""
import ctypes as C

import numpy as np
import pytest

import grouplasso_restated as G
import penalty_restated as R

pytestmark = pytest.mark.gpu

SIZES = R.SIZES
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


def _solve(gpu, p, opts):
    pen = p["pen"]
    o = dict(opts, **pen.options())
    if pen.sizes is not None:
        return gpu.grouplasso(p["D"], p["s"], p["lam"], pen.sizes, o)
    return gpu.lasso(p["D"], p["s"], p["lam"], o)


_REF = {}


def _run_both(gpu, p, opts, key=None):
    """the device run and the restatement's; a reference is computed once per (fixture, options) and shared"""
    got = _solve(gpu, p, opts)
    ro = {k: v for k, v in opts.items() if k not in ("xsolve", "record_history")}
    if key is None or key not in _REF:
        ref = R.run(p["D"], p["s"], p["lam"], p["pen"], ro)
        if key is None:
            return got, ref
        _REF[key] = ref
    return got, _REF[key]


# ------------------------------------------------------------------------------------------- the prox alone
def _device_prox(gpu, v, pen, tau, t, rho):
    """admm_op_penalty_prox: without groups lambda_over_rho is the l1 threshold; with groups it is theirs and the l1
    threshold is desc.l1 / rho"""
    L = gpu._lib
    lib = L.load()
    v = np.ascontiguousarray(v, dtype=np.float64)
    out = np.full(v.size, np.nan)
    w = None if pen.w is None else np.ascontiguousarray(pen.w)
    grouped = pen.sizes is not None
    sz = np.ascontiguousarray(pen.sizes if grouped else [], dtype=np.int64)
    gw = None if pen.gw is None else np.ascontiguousarray(pen.gw)
    d = L.PenaltyDesc(None if w is None else L.as_dp(w), tau * rho if grouped else 0.0, pen.ridge, pen.nonnegative)
    L.check(lib.admm_op_penalty_prox(L.as_dp(v), v.size, sz.ctypes.data_as(C.POINTER(C.c_int64)) if grouped else None,
                                     sz.size, None if gw is None else L.as_dp(gw), float(t if grouped else tau),
                                     C.byref(d), float(rho), L.as_dp(out)))
    return out


def _check_prox(gpu, v, pen, tau, t, rho):
    """per element |out_i - exact_i| <= (p_g + 12)*eps*(|v_i| + tau_i)  (penalty_restated.bound_ratio)"""
    if pen.sizes is not None:  # the device forms tau = desc.l1 / rho: hand the restatement that very number
        tau = (tau * rho) / rho
    out = _device_prox(gpu, v, pen, tau, t, rho)
    assert np.isfinite(out).all()
    exact = R.prox(v, pen, tau, t, rho, dtype=np.longdouble)
    worst = R.bound_ratio(v, out, exact, pen, tau)
    print(f"n = {len(v)}, groups = {pen.sizes is not None}, tau = {tau:g}: worst |out - exact| / bound = {worst:.3f}")
    assert worst <= 1.0
    return out, exact


CASES = ["tau=0", "tau=1e-12", "median", "above", "zero-weight", "nonnegative"]


def _case(case, v):
    n = v.size
    tau = {"tau=0": 0.0, "tau=1e-12": 1e-12, "above": 2.0 * float(np.max(np.abs(v)))}.get(case, float(np.median(np.abs(v))))
    w = None
    if case == "zero-weight":
        w = np.random.default_rng(13).uniform(0.5, 2.0, n)
        w[n // 2] = 0.0
    return tau, w


@pytest.mark.parametrize("case", CASES)
def test_prox_without_groups_against_long_double(gpu, case):
    for n in (1, 127, 128, 129, 700):
        v = np.random.default_rng(11).standard_normal(n)
        tau, w = _case(case, v)
        for nonneg in ((1,) if case == "nonnegative" else (0, 1) if case == "tau=0" else (0,)):
            pen = R.Penalty(l1weights=w, nonnegative=nonneg)
            out, exact = _check_prox(gpu, v, pen, tau, 0.0, 1.0)
            if case == "tau=0":
                assert np.array_equal(out, np.maximum(v, 0.0) if nonneg else v)  # bit for bit
            if case == "above":
                assert np.array_equal(out, np.zeros(n))
            if case == "median" and n > 1:
                assert np.any(exact == 0) and np.any(exact != 0)
            if case == "zero-weight":
                assert out[n // 2] == v[n // 2]  # the unpenalised coefficient passes unchanged
            if case == "nonnegative":
                assert np.all(out >= 0) and np.array_equal(out == 0, v <= tau)
        # the ridge factor on top, rho != 1
        _check_prox(gpu, v, R.Penalty(l1weights=w, ridge=0.7, nonnegative=int(case == "nonnegative")), tau, 0.0, 1.3)


@pytest.mark.parametrize("case", CASES)
def test_prox_with_groups_against_long_double(gpu, case):
    v = np.random.default_rng(11).standard_normal(700)
    tau, w = _case(case, v)
    gw = np.sqrt(np.asarray(SIZES, dtype=np.float64))
    off = G.offsets(SIZES)
    nonneg = int(case == "nonnegative")
    for t in (0.0, 0.35):
        pen = R.Penalty(l1weights=w, nonnegative=nonneg, sizes=SIZES, groupweights=gw)
        out, exact = _check_prox(gpu, v, pen, tau, t, 1.0)
        if case == "tau=0" and t == 0.0:
            assert np.array_equal(out, v)
        if case == "above":
            assert np.array_equal(out, np.zeros(700))
        if case == "median" and t > 0:
            zero = [not np.any(exact[off[g]:off[g + 1]]) for g in range(len(SIZES))]
            assert any(zero) and not all(zero)
            assert any(np.any(exact[off[g]:off[g + 1]] == 0) for g in range(len(SIZES)) if not zero[g])
    _check_prox(gpu, v, R.Penalty(l1weights=w, ridge=0.7, nonnegative=nonneg, sizes=SIZES, groupweights=gw), tau, 0.35, 1.3)
    if case == "tau=0":
        out, _ = _check_prox(gpu, v, R.Penalty(nonnegative=1, sizes=SIZES), 0.0, 0.0, 1.0)
        assert np.array_equal(out, np.maximum(v, 0.0))


def test_prox_refuses_bad_arguments(gpu):
    L = gpu._lib
    v = np.ones(8)
    for pen, tau in ((R.Penalty(l1weights=[1.0] * 7 + [-1.0]), 0.5), (R.Penalty(l1weights=[1.0] * 7 + [np.nan]), 0.5),
                     (R.Penalty(ridge=-1.0), 0.5), (R.Penalty(nonnegative=2), 0.5), (R.Penalty(), -0.5),
                     (R.Penalty(sizes=[3, 4]), 0.5)):
        with pytest.raises(gpu.AdmmError) as ei:
            _device_prox(gpu, v, pen, tau, 0.5, 1.0)
        assert ei.value.code == L.E_INVALID


# ------------------------------------------------------------------------------------------- full runs
@pytest.fixture(scope="module")
def fixtures(gpu):
    out = {}
    for which, rows in (("tall", 1024), ("wide", 512)):
        for kind in R.KINDS:
            out[which, kind] = R.fixture(gpu.synth, kind, rows, 700, R.SEEDS[which])
    return out


@pytest.mark.parametrize("which", ["tall", "wide"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_run_to_the_stop(gpu, fixtures, which, kind):
    p = fixtures[which, kind]
    got, ref = _run_both(gpu, p, dict(objevals=1), key=(which, kind, "stop"))
    assert 5 <= ref["steps"] < 1000
    _same_run(got, ref)
    plain = gpu.lasso(p["D"], p["s"], p["lam"], dict(objevals=1))
    assert not np.allclose(plain["zopt"], got["zopt"], rtol=1e-6, atol=1e-9)  # a build that ignores the penalty differs


@pytest.mark.parametrize("kind", ["all", "sparsegroup"])
@pytest.mark.parametrize("opts,hist,steps", [
    (dict(maxiters=30, domaxiters=1), PLAIN, 30), (dict(relax=1.6), PLAIN, None),
    (dict(fast=1, fasttype="strong"), STRONG, None), (dict(fast=1, fasttype="weak"), WEAK, None),
    (dict(xsolve="trsv"), PLAIN, None), (dict(xsolve="inverse"), PLAIN, None),
    (dict(record_history=0), ("pnorm", "dnorm", "perr", "derr", "objevals"), None),
], ids=["forced30", "relax", "strong", "weak", "trsv", "inverse", "nohistory"])
def test_variants(gpu, fixtures, kind, opts, hist, steps):
    """the combined cases (weights + ridge + sign; sparse-group + ridge) on 1024 x 700"""
    p = fixtures["tall", kind]
    plainkey = "stop" if set(opts) <= {"xsolve", "record_history"} else tuple(sorted(opts.items()))
    got, ref = _run_both(gpu, p, dict(opts, objevals=1), key=("tall", kind, plainkey))
    if "xsolve" in opts:
        assert got["engine_info"]["xsolve_used"] == opts["xsolve"]
    if "record_history" in opts:
        assert "xvals" not in got
    if opts.get("fasttype") == "weak":
        _weak_run(got, ref)
        return
    _same_run(got, ref, steps=steps, hist=hist)


def _weak_run(got, ref):
    """Weak fast ADMM has no stop test of its own (admm.m records no norms there), so "to the stop" is all 1000
    iterations, and the iterates have converged to rounding long before: from there on the restart decision
    d < restart*dprev compares d = ||u - uhat||^2/rho + rho*||z - v||^2, differences of vectors that agree to their last
    bits, and the REFERENCE's own avals / dvals / restarted are decided by its rounding (it restarts on almost every
    iteration there).  d is a sum of 2n squares of differences, each with an absolute error of a few eps*max(|z|, |u|):
    below floor = 64*n*eps^2*max(|z|, |u|)^2*(rho + 1/rho) it is noise.  The three decision histories are compared up to
    the first iteration at which the reference's d is below that floor (76 and 134 for the two fixtures, of 1000; the
    first restarts of the reference fall at 39 and 158), every iterate history and the objective over the whole run."""
    n, rho = ref["zopt"].size, 1.0
    scale = max(float(np.max(np.abs(ref["zopt"]))), float(np.max(np.abs(ref["uopt"]))))
    floor = 64 * n * R.EPS ** 2 * scale ** 2 * (rho + 1.0 / rho)
    d = np.asarray(ref["dvals"], dtype=np.float64)
    k0 = int(np.argmax(d <= floor)) if np.any(d <= floor) else d.size
    first = np.nonzero(np.asarray(got["avals"]) != np.asarray(ref["avals"]))[0]
    print(f"decision histories compared over the first {k0} of {d.size} iterations (floor {floor:.3e}); first iteration "
          f"whose avals differ: {int(first[0]) if first.size else None}")
    assert k0 >= 50 and np.any(np.asarray(ref["restarted"])[:k0 + 30] != 0)
    _same_run(got, ref, hist=("xvals", "zvals", "uvals", "vvals", "uhatvals", "objevals"))
    for key in ("avals", "dvals", "restarted"):
        _err(key, np.asarray(got[key])[:k0], np.asarray(ref[key])[:k0])


@pytest.mark.parametrize("kind", ["all", "sparsegroup"])
def test_forced_30_on_the_fat_shape(gpu, fixtures, kind):
    got, ref = _run_both(gpu, fixtures["wide", kind], dict(objevals=1, maxiters=30, domaxiters=1))
    _same_run(got, ref, steps=30)


@pytest.mark.parametrize("kind", ["all", "sparsegroup"])
def test_warm_start(gpu, fixtures, kind):
    rng = np.random.default_rng(8)
    o = dict(objevals=1, x0=rng.standard_normal(700), z0=rng.standard_normal(700), u0=0.1 * rng.standard_normal(700))
    got, ref = _run_both(gpu, fixtures["tall", kind], o)
    _same_run(got, ref)


@pytest.mark.parametrize("form", ["inverse", "one"])
def test_partial_rows_of_the_x_solve(gpu, form, monkeypatch):
    """n = 1600 >= 1536: the x-solve leaves its partial rows to the element update -- the packed lower-triangle product
    (N-part and T-part rows, deferred finalize) and the one-block triangular solves (rows from the diagonal tile on).
    12 forced iterations of plain and of strong fast ADMM, without groups and with groups that cross the tiles"""
    if form == "one":
        monkeypatch.setenv("ADMM_TRSV_FORM", "one")
    xs = "inverse" if form == "inverse" else "trsv"
    for kind in ("all", "sparsegroup"):
        p = R.fixture(gpu.synth, kind, 2000, 1600, R.SEEDS["rows"], sizes=SIZES + [500, 400])
        for extra, hist in ((dict(), PLAIN), (dict(fast=1, fasttype="strong"), STRONG)):
            o = dict(extra, objevals=1, maxiters=12, domaxiters=1, xsolve=xs)
            got, ref = _run_both(gpu, p, o, key=("rows", kind, tuple(sorted(extra.items()))))
            info = got["engine_info"]
            assert info["xsolve_used"] == xs and (form != "one" or info["trsv_blocks"] == 1)
            _same_run(got, ref, steps=12, hist=hist)


# ------------------------------------------------------------------------------------------- launches, setter
def _engine_run(gpu, eng, n, **kw):
    L = gpu._lib
    eng.run(maxiters=30, domaxiters=1, objevals=1, **kw)
    return {k: eng.fetch(f, n) for k, f in (("x", L.F_XOPT), ("z", L.F_ZOPT), ("u", L.F_UOPT))} | \
        {k: eng.fetch(f, 30) for k, f in (("pnorm", L.F_PNORM), ("dnorm", L.F_DNORM), ("obj", L.F_OBJEVALS))}


def test_launch_counts_reproducibility_and_setter_edges(gpu, fixtures):
    """30 forced iterations on one engine: the same launches per iteration with and without a penalty, with and without
    groups; a repeat run is bitwise identical; a refused call changes nothing; set_penalty(None) gives plain lasso back
    bit for bit, in either order with set_groups"""
    L = gpu._lib
    p, pg = fixtures["tall", "all"], fixtures["tall", "sparsegroup"]
    D, s, lam, pen = p["D"], p["s"], p["lam"], p["pen"]
    kinds = (L.K_PROX, L.K_FINALIZE, L.K_XSOLVE)
    eng = gpu.Engine(L.PROB_LASSO, D=D, s=s, lam=lam)
    try:
        eng.set_profiling(list(kinds))
        _engine_run(gpu, eng, 700)  # (an engine's first objevals run calibrates the objective's form: other launches)
        plain = _engine_run(gpu, eng, 700)
        counts = [eng.kernel_time(k)[1] for k in kinds]
        assert counts[0] == 30
        assert eng.penalty() == dict(l1=0.0, ridge=0.0, nonnegative=0, has_l1weights=False)
        eng.set_penalty(pen.w, pen.ridge, pen.nonnegative)
        assert eng.penalty() == dict(l1=0.0, ridge=pen.ridge, nonnegative=1, has_l1weights=True)
        first = _engine_run(gpu, eng, 700)
        assert [eng.kernel_time(k)[1] for k in kinds] == counts
        ref = R.run(D, s, lam, pen, dict(objevals=1, maxiters=30, domaxiters=1))
        _err("penalised zopt", first["z"], ref["zopt"])
        _err("penalised objevals", first["obj"], ref["objevals"])
        assert not np.array_equal(first["z"], plain["z"])
        again = _engine_run(gpu, eng, 700)
        for k in first:
            assert np.array_equal(again[k], first[k]), k  # bitwise reproducible
        # refused calls leave the engine as it is
        for bad in (dict(l1weights=np.r_[np.ones(699), -1.0]), dict(l1weights=np.r_[np.ones(699), np.nan]),
                    dict(ridge=-1.0), dict(ridge=float("inf")), dict(l1=-0.1), dict(nonnegative=2)):
            with pytest.raises(gpu.AdmmError) as ei:
                eng.set_penalty(**bad)
            assert ei.value.code == L.E_INVALID
        with pytest.raises(ValueError):
            eng.set_penalty(np.ones(699))
        assert eng.penalty() == dict(l1=0.0, ridge=pen.ridge, nonnegative=1, has_l1weights=True)
        still = _engine_run(gpu, eng, 700)
        for k in first:
            assert np.array_equal(still[k], first[k]), k
        # groups on top (the sparse-group fixture shares D; its own s and lambda do not matter for the launch count)
        gpen = pg["pen"]
        eng.set_groups(gpen.sizes, gpen.gw)
        eng.set_penalty(None, gpen.ridge, 0, gpen.l1)
        sg = _engine_run(gpu, eng, 700)
        assert [eng.kernel_time(k)[1] for k in kinds] == counts
        sg2 = _engine_run(gpu, eng, 700)
        for k in sg:
            assert np.array_equal(sg2[k], sg[k]), k
        # the other order gives the same engine: penalty first, groups second
        eng.set_groups(None)
        eng.set_penalty(None)
        eng.set_penalty(None, gpen.ridge, 0, gpen.l1)
        eng.set_groups(gpen.sizes, gpen.gw)
        sg3 = _engine_run(gpu, eng, 700)
        for k in sg:
            assert np.array_equal(sg3[k], sg[k]), k
        refg = R.run(D, s, lam, gpen, dict(objevals=1, maxiters=30, domaxiters=1))
        _err("sparse-group zopt", sg["z"], refg["zopt"])
        _err("sparse-group objevals", sg["obj"], refg["objevals"])
        # defaults restored: penalty off with groups still on = group lasso; then groups off = plain lasso, bit for bit
        eng.set_penalty(None)
        grp = _engine_run(gpu, eng, 700)
        eng.set_groups(None)
        back = _engine_run(gpu, eng, 700)
        for k in plain:
            assert np.array_equal(back[k], plain[k]), k
        eng.set_penalty(pen.w, pen.ridge, pen.nonnegative)
        eng.set_groups(gpen.sizes, gpen.gw)
        eng.set_groups(None)
        eng.set_penalty(None)
        back2 = _engine_run(gpu, eng, 700)
        eng.set_groups(gpen.sizes, gpen.gw)
        grp2 = _engine_run(gpu, eng, 700)
        for k in plain:
            assert np.array_equal(back2[k], plain[k]), k
            assert np.array_equal(grp2[k], grp[k]), k
    finally:
        eng.close()


def test_set_penalty_on_an_svm_engine_is_unsupported(gpu):
    L = gpu._lib
    p = gpu.synth.svm_problem(0)
    eng = gpu.Engine(L.PROB_LINEARSVM, D=p["D"], ell=p["ell"], Cval=p["C"])
    try:
        with pytest.raises(gpu.AdmmError) as ei:
            eng.set_penalty(ridge=0.5)
        assert ei.value.code == L.E_UNSUPPORTED
    finally:
        eng.close()


def test_a_zming_callback_wins_over_the_penalty(gpu):
    """the caller's z-update replaces the penalised one as it replaces the l1 prox"""
    import torch
    p = gpu.synth.lasso_problem(2, 256, 64)
    args = dict(D=p["D"], s=p["s"], ridge=0.5, nonnegative=1, l1weights=np.linspace(0.5, 2.0, 64))
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
def test_elasticnettest(gpu, seed):
    results, test = gpu.testers.elasticnettest(seed=seed)
    print(f"objopt {test['objopt']:.6f} < testobj {test['testobj']:.6f}, {test['steps']} steps")
    assert test["failed"] == 0
    ref = R.run(test["D"], test["s"], test["lambda"], R.Penalty(ridge=test["ridge"]), dict(objevals=1))
    _same_run(results, ref)


def test_mex_gateway_carries_the_family(gpu, tmp_path_factory):
    """args.l1weights / ridge / nonnegative / l1 reach the setter through the binding layer with no change to the gateway"""
    from mexharness import Harness, MexError, build
    mex = Harness(build(tmp_path_factory.mktemp("mexpenalty")))
    sizes = [1, 20, 7, 36]
    p = R.fixture(gpu.synth, "sparsegroup", 256, 64, 10, sizes=sizes)
    D, s, lam, pen = p["D"], p["s"], p["lam"], p["pen"]
    w = np.random.default_rng(14).uniform(0.5, 2.0, 64)
    options = dict(objevals=1, A=1, At=1, m=64, nA=64, nB=64, B=-1, c=0, parallel="none")
    # without groups: weights, ridge and the sign constraint
    args = dict(D=D, s=s, m=256, n=64, parallel=0, rho=1.0, l1weights=w, ridge=0.5, nonnegative=1.0)
    args["lambda"] = lam
    got = mex.call("solve", "lasso", args, options, dict(objnative=1, s=s))
    ref = gpu.lasso(D, s, lam, dict(objevals=1, l1weights=w, ridge=0.5, nonnegative=1))
    assert int(got["steps"]) == int(ref["steps"])
    for key in ("xopt", "zopt", "zvals", "objevals"):
        _err(key, got[key], ref[key], 1e-12)
    assert np.min(ref["zopt"]) == 0.0
    # sparse-group: l1 beside the groups
    argsg = dict(D=D, s=s, m=256, n=64, parallel=0, rho=1.0, groups=np.asarray(sizes, dtype=np.float64),
                 groupweights=pen.gw, l1=pen.l1, ridge=pen.ridge, l1weights=w)
    argsg["lambda"] = lam
    gotg = mex.call("solve", "lasso", argsg, options, dict(objnative=1, s=s))
    refg = gpu.grouplasso(D, s, lam, sizes, dict(objevals=1, groupweights=pen.gw, l1=pen.l1, ridge=pen.ridge, l1weights=w))
    assert int(gotg["steps"]) == int(refg["steps"])
    for key in ("xopt", "zopt", "zvals", "objevals"):
        _err(key, gotg[key], refg[key], 1e-12)
    assert not np.allclose(refg["zopt"], ref["zopt"], rtol=1e-6, atol=1e-9)
    args["l1weights"] = w[:63]
    with pytest.raises(MexError):
        mex.call("solve", "lasso", args, options, dict(objnative=1, s=s))
