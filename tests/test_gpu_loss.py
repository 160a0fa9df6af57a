"""The loss family of the LAD and Huber engines on the device: the prox operator against long double,
runs of every iteration form against the restatement (tests/loss_restated.py) at the project's per-iteration tolerance
1e-7, the launch counts, reproducibility, the setter's edges, the tester and the MEX gateway.  tests/test_loss_host.py
checks the restatement itself on the CPU."""
import numpy as np
import pytest

import loss_restated as R

pytestmark = pytest.mark.gpu

PLAIN = ("xvals", "zvals", "uvals", "pnorm", "dnorm", "perr", "derr", "objevals")
STRONG = PLAIN + ("vvals", "uhatvals", "avals")
WEAK = ("xvals", "zvals", "uvals", "vvals", "uhatvals", "objevals", "avals", "dvals", "restarted")  # (admm.m records no norms there)
NODUAL = ("xvals", "zvals", "uvals", "pnorm", "perr", "objevals")  # (nodualerror: dnorm, derr are NaN on both sides)
SHAPES = dict(small=(300, 40), onepass=(16421, 400))  # 16421 x 400: 52.5 MB, n <= 448, a last row block of 37 rows


def _err(name, got, ref, tol=1e-7):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert not np.isnan(got).any() and not np.isnan(ref).any(), f"{name}: NaN"
    err = float(np.max(np.abs(got - ref)) / max(1e-300, np.max(np.abs(ref))))
    print(f"{name}: relative error {err:.3e} (bound {tol:g})")
    assert err < tol, f"{name}: relative error {err:.3e} >= {tol:g}"


def _same_run(got, ref, hist, tol=1e-7):
    """every history of the case (a missing one is a failure), the final iterates, the objective and the step count
    (maxiters = 30; a run under nodualerror may meet its primal tolerance earlier, on both sides)"""
    assert 1 <= int(got["steps"]) == int(ref["steps"]) <= 30, (got["steps"], ref["steps"])
    for key in hist:
        assert key in got and key in ref, key
        _err(key, got[key], ref[key], tol)
    for key in ("xopt", "zopt", "uopt"):
        _err(key, got[key], ref[key], tol)
    _err("objopt", [got["objopt"]], [ref["objopt"]], tol)


def _solve(gpu, D, s, loss, opts):
    return getattr(gpu, loss.kind)(D, s, dict(opts, **loss.options()))


# ------------------------------------------------------------------------------------------- the prox alone
def _device_prox(gpu, v, loss, rho):
    import ctypes as C
    L = gpu._lib
    v = np.ascontiguousarray(v, dtype=np.float64)
    out = np.full(v.size, np.nan)
    w = None if loss.w is None else np.ascontiguousarray(loss.w)
    d = L.LossDesc(None if w is None else L.as_dp(w), loss.a, loss.b, loss.eps, loss.delta)
    L.check(L.load().admm_op_loss_prox(L.as_dp(v), v.size, L.PROB_LAD if loss.kind == "lad" else L.PROB_HUBERFIT,
                                       C.byref(d), float(rho), L.as_dp(out)))
    return out


def _prox_members(n):
    w = np.random.default_rng(13).uniform(0.5, 2.0, n)
    w[n // 2] = 0.0
    w[3] = 0.0
    return {
        "lad-defaults": R.Loss("lad"),
        "quantile-weights": R.Loss("lad", weights=w, slopes=(0.9, 0.1)),
        "svr": R.Loss("lad", epsilon=0.3),
        "svr-asym-weights": R.Loss("lad", weights=w, slopes=(1.5, 0.25), epsilon=0.7),
        "huber-defaults": R.Loss("huberfit"),
        "huber-asym-weights": R.Loss("huberfit", weights=w, slopes=(1.5, 0.5), delta=0.5),
    }


@pytest.mark.parametrize("rho", [0.3, 1.0, 41.0])
@pytest.mark.parametrize("name", list(_prox_members(8)))
def test_prox_against_long_double(gpu, name, rho):
    """admm_op_loss_prox at len = 1000 (no multiple of the block), v in every branch and exactly on every breakpoint: per
    element |out - exact| <= 12*eps*(|v_i| + t_a + t_b + epsilon); exact where the formula says so -- the dead zone,
    w = 0, the flats at +-epsilon"""
    n = 1000
    loss = _prox_members(n)[name]
    v = R.breakpoint_vector(loss, rho, n=n)
    out = _device_prox(gpu, v, loss, rho)
    assert np.isfinite(out).all()
    exact = R.prox(v, loss, rho, dtype=np.longdouble)
    worst = R.bound_ratio(v, out, exact, loss, rho)
    print(f"{name}, rho = {rho:g}: worst |out - exact| / bound = {worst:.3f}")
    assert worst <= 1.0
    w = np.ones(n) if loss.w is None else loss.w
    assert np.array_equal(out[w == 0], v[w == 0])
    if loss.kind == "lad":
        ta, tb = (w * loss.a) / rho, (w * loss.b) / rho
        dead = (v > -loss.eps) & (v < loss.eps)
        flat_hi = (v >= loss.eps) & (v <= loss.eps + ta) & (w > 0)
        flat_lo = (v >= -loss.eps - tb) & (v <= -loss.eps) & (w > 0) & ~flat_hi
        assert flat_hi.any() and flat_lo.any() and (dead.any() or loss.eps == 0)
        assert np.array_equal(out[dead], v[dead])
        assert np.all(out[flat_hi] == loss.eps) and np.all(out[flat_lo] == -loss.eps)


def test_prox_refuses_bad_arguments(gpu):
    L = gpu._lib
    v = np.ones(8)
    for kind, kw in (("lad", dict(slopes=(0.0, 1.0))), ("lad", dict(slopes=(1.0, -1.0))), ("lad", dict(epsilon=-0.1)),
                     ("lad", dict(delta=0.5)), ("huberfit", dict(epsilon=0.1)), ("huberfit", dict(delta=0.0)),
                     ("lad", dict(weights=np.r_[np.ones(7), -1.0])), ("lad", dict(weights=np.r_[np.ones(7), np.nan]))):
        with pytest.raises(gpu.AdmmError) as ei:
            _device_prox(gpu, v, R.Loss(kind, **kw), 1.0)
        assert ei.value.code == L.E_INVALID, (kind, kw)


# ------------------------------------------------------------------------------------------- whole runs
@pytest.fixture(scope="module")
def problems(gpu):
    out = {}
    for shape, (m, n) in SHAPES.items():
        D, s = R.regression(gpu.synth, m, n, 11 if shape == "small" else 12)
        out[shape] = (D, s, {name: R.member(name, m) for name in R.MEMBERS})
    return out


FORMS = {
    "plain": ("small", dict(objevals=1, maxiters=30), PLAIN),
    "relax": ("small", dict(objevals=1, maxiters=30, relax=1.5), PLAIN),
    "strong": ("small", dict(objevals=1, maxiters=30, fast=1, fasttype="strong"), STRONG),
    "weak": ("small", dict(objevals=1, maxiters=30, fast=1, fasttype="weak"), WEAK),
    "tail": ("small", dict(objevals=1, maxiters=30, nodualerror=1), NODUAL),
    "onepass": ("onepass", dict(objevals=1, maxiters=30, nodualerror=1), NODUAL),
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", R.MEMBERS)
def test_runs_against_the_restatement(gpu, problems, name, form):
    """maxiters = 30 in every iteration form: plain, relaxed, fast ADMM with strong and weak restarts (launch_prox), the
    fused tail under nodualerror (launch_prox_fin) and the one-pass kernel at 16421 x 400 (ad_onepass_kernel)"""
    shape, opts, hist = FORMS[form]
    D, s, members = problems[shape]
    loss = members[name]
    got = _solve(gpu, D, s, loss, opts)
    ref = R.run(loss.kind, D, s, loss, dict(opts))
    _same_run(got, ref, hist)
    if "dnorm" not in hist and form in ("tail", "onepass"):
        assert np.isnan(got["dnorm"]).all()
    default = getattr(gpu, loss.kind)(D, s, dict(opts))
    assert not np.allclose(default["zopt"], got["zopt"], rtol=1e-3, atol=1e-6)  # the member shapes the iterates


# ------------------------------------------------------------------------------------------- launches, setter
def _engine_run(gpu, eng, m, n, **kw):
    L = gpu._lib
    eng.run(maxiters=30, domaxiters=1, objevals=1, **kw)
    return {k: eng.fetch(f, c) for k, f, c in (("x", L.F_XOPT, n), ("z", L.F_ZOPT, m), ("u", L.F_UOPT, m))} | \
        {k: eng.fetch(f, 30) for k, f in (("pnorm", L.F_PNORM), ("obj", L.F_OBJEVALS))}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", R.MEMBERS)
def test_launch_counts_determinism_and_round_trip(gpu, problems, name, shape):
    """nodualerror = 1 on one engine: the family launches what the default engine launches, per kernel class; two runs
    are bitwise equal; a refused call changes nothing; set_loss(None) gives the default engine back bit for bit"""
    L = gpu._lib
    D, s, members = problems[shape]
    m, n = D.shape
    loss = members[name]
    code = L.PROB_LAD if loss.kind == "lad" else L.PROB_HUBERFIT
    kinds = (L.K_PROX, L.K_FINALIZE, L.K_XSOLVE, L.K_GEMV_N, L.K_GEMV_T)
    fresh = gpu.Engine(code, D=D, s=s)
    eng = gpu.Engine(code, D=D, s=s)
    try:
        want = _engine_run(gpu, fresh, m, n, nodualerror=1)
        eng.set_profiling(list(kinds))
        _engine_run(gpu, eng, m, n, nodualerror=1)
        counts = [eng.kernel_time(k)[1] for k in kinds]
        assert counts[0] == 30 and (counts[3] == 0) == (shape == "onepass")
        assert eng.loss() == dict(slopes=(1.0, 1.0), epsilon=0.0, delta=1.0, has_weights=False)
        eng.set_loss(loss.w, (loss.a, loss.b), loss.eps, loss.delta)
        assert eng.loss() == dict(slopes=(loss.a, loss.b), epsilon=loss.eps, delta=loss.delta, has_weights=loss.w is not None)
        first = _engine_run(gpu, eng, m, n, nodualerror=1)
        assert [eng.kernel_time(k)[1] for k in kinds] == counts
        assert not np.array_equal(first["z"], want["z"])
        again = _engine_run(gpu, eng, m, n, nodualerror=1)
        for k in first:
            assert np.array_equal(again[k], first[k]), k  # bitwise reproducible
        for bad in (dict(weights=np.r_[np.ones(m - 1), -1.0]), dict(weights=np.r_[np.ones(m - 1), np.inf]),
                    dict(slopes=(0.0, 1.0)), dict(slopes=(1.0, np.nan)), dict(epsilon=-1.0), dict(delta=-1.0),
                    dict(delta=0.5) if loss.kind == "lad" else dict(epsilon=0.5)):
            with pytest.raises(gpu.AdmmError) as ei:
                eng.set_loss(**bad)
            assert ei.value.code == L.E_INVALID, bad
        with pytest.raises(ValueError):
            eng.set_loss(np.ones(m - 1))
        still = _engine_run(gpu, eng, m, n, nodualerror=1)
        for k in first:
            assert np.array_equal(still[k], first[k]), k
        eng.set_loss(None)
        assert eng.loss() == dict(slopes=(1.0, 1.0), epsilon=0.0, delta=1.0, has_weights=False)
        back = _engine_run(gpu, eng, m, n, nodualerror=1)
        for k in want:
            assert np.array_equal(back[k], want[k]), k
        if shape == "small":  # and with the dual residual (launch_prox)
            eng.set_profiling(False)
            want2 = _engine_run(gpu, fresh, m, n)
            eng.set_loss(loss.w, (loss.a, loss.b), loss.eps, loss.delta)
            a, b = _engine_run(gpu, eng, m, n), _engine_run(gpu, eng, m, n)
            eng.set_loss(None)
            back2 = _engine_run(gpu, eng, m, n)
            for k in want2:
                assert np.array_equal(a[k], b[k]) and np.array_equal(back2[k], want2[k]), k
    finally:
        eng.close()
        fresh.close()


def test_set_loss_refusals(gpu):
    """a wrong problem (ADMM_E_INVALID), the generic callback engine and an engine with a communicator (UNSUPPORTED)"""
    from admm_project_amd import parallel
    L = gpu._lib
    p = gpu.synth.svm_problem(0)
    eng = gpu.Engine(L.PROB_LINEARSVM, D=p["D"], ell=p["ell"], Cval=p["C"])
    q = gpu.synth.lasso_problem(0, 64, 16)
    lasso = gpu.Engine(L.PROB_LASSO, D=q["D"], s=q["s"], lam=q["lam"])
    D, s = R.regression(gpu.synth, 64, 8, 1)
    generic = gpu.Engine(L.PROB_LAD, D=D, s=s, xsolve=L.XSOLVE_CALLBACK)
    comm = parallel.Comm(parallel.unique_id(), 0, 1, device=0, transport="rccl")
    sharded = gpu.Engine(L.PROB_LAD, D=D, s=s, comm=comm)
    try:
        for e, code in ((eng, L.E_INVALID), (lasso, L.E_INVALID), (generic, L.E_UNSUPPORTED), (sharded, L.E_UNSUPPORTED)):
            with pytest.raises(gpu.AdmmError) as ei:
                e.set_loss(slopes=(0.9, 0.1))
            assert ei.value.code == code
        with pytest.raises(ValueError):  # lad() itself refuses options.comm beside the family, before the engine
            gpu.lad(D, s, dict(comm=comm, slopes=(0.9, 0.1)))
        with pytest.raises(gpu.AdmmError) as ei:
            gpu.getproxops("LAD", dict(D=D, s=s, comm=comm, tau=0.9))
        assert ei.value.code == L.E_UNSUPPORTED
    finally:
        for e in (eng, lasso, generic, sharded):
            e.close()
        comm.close()


def test_a_zming_callback_wins_over_the_loss(gpu):
    """the caller's z-update replaces the family's as it replaces the l1 prox"""
    import torch
    D, s = R.regression(gpu.synth, 300, 40, 11)
    m, n = D.shape
    gx, _, _ = gpu.getproxops("LAD", dict(D=D, s=s, tau=0.9, weights=np.linspace(0.5, 2.0, m)))
    st = torch.as_tensor(s, device="cuda")
    Dt = torch.as_tensor(np.ascontiguousarray(D), device="cuda")
    zmin = lambda x, _z, u, rho: (lambda v: torch.sign(v) * torch.clamp(torch.abs(v) - 1.0 / rho, min=0.0))(Dt @ x + u - st)
    got = gpu.admm(gx, zmin, dict(A=D, At=D.T, B=-1, c=s, m=m, nA=n, nB=m, maxiters=30))
    ref = gpu.lad(D, s, dict(maxiters=30))
    assert int(got["steps"]) == int(ref["steps"])
    for key in ("xvals", "zvals", "uvals", "pnorm", "dnorm", "xopt", "zopt"):
        _err(key, got[key], ref[key], 1e-9)


# ------------------------------------------------------------------------------------------- tester, gateway
def test_quantileregtest(gpu):
    results, test = gpu.testers.quantileregtest(seed=0)
    print(f"tau = {test['tau']}: #(z<0) = {test['negative']}, #(z==0) = {test['zero']}, slack {test['slack']:g}, "
          f"{test['steps']} steps, objopt {test['objopt']:.6f}")
    assert test["failed"] == 0


def test_mex_gateway_carries_the_family(gpu, tmp_path_factory):
    """args.weights / tau / slopes / epsilon / delta reach the setter through the binding layer with no change to the
    gateway"""
    from mexharness import Harness, MexError, build
    mex = Harness(build(tmp_path_factory.mktemp("mexloss")))
    D, s = R.regression(gpu.synth, 300, 40, 11)
    m, n = D.shape
    w = np.random.default_rng(14).uniform(0.5, 2.0, m)
    Rf = np.linalg.cholesky(D.T @ D)
    options = dict(objevals=1, A=D, At=D.T, B=-1, c=s, m=m, nA=n, nB=m, maxiters=30)
    got = mex.call("solve", "lad", dict(R=Rf, D=D, s=s, weights=w, tau=0.9, epsilon=0.1), options, dict(objnative=1))
    ref = gpu.lad(D, s, dict(objevals=1, maxiters=30, weights=w, tau=0.9, epsilon=0.1))
    assert int(got["steps"]) == int(ref["steps"])
    for key in ("xopt", "zopt", "zvals", "objevals"):
        _err(key, got[key], ref[key], 1e-12)
    goth = mex.call("solve", "huberfit", dict(R=Rf, D=D, s=s, weights=w, slopes=np.array([1.5, 0.5]), delta=0.5), options,
                    dict(objnative=1))
    refh = gpu.huberfit(D, s, dict(objevals=1, maxiters=30, weights=w, slopes=(1.5, 0.5), delta=0.5))
    for key in ("xopt", "zopt", "zvals", "objevals"):
        _err(key, goth[key], refh[key], 1e-12)
    plain = gpu.lad(D, s, dict(objevals=1, maxiters=30))
    assert not np.allclose(plain["zopt"], ref["zopt"], rtol=1e-3, atol=1e-6)
    with pytest.raises(MexError):
        mex.call("solve", "lad", dict(R=Rf, D=D, s=s, weights=w[:m - 1]), options, dict(objnative=1))
    with pytest.raises(MexError):
        mex.call("solve", "lad", dict(R=Rf, D=D, s=s, tau=0.3, slopes=np.array([0.3, 0.7])), options, dict(objnative=1))
