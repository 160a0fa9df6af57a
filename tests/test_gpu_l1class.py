"""The sparse linear classifier on the device against the restated run (l1class_restated, which
test_l1class_host checks against the optimality conditions): per iteration from shared z0 / u0 with domaxiters = 1 --
pnorm, perr, the dual residual and its tolerance, the objective history, xopt / zopt / uopt -- over the shapes at which
the kernels take another path, then two chunks (bits, freezing), the penalty and cost family, nodualerror, the
triangular solves, a converged run, the path, the refusals of the C ABI and a bare C-ABI call sequence.

Parity bound: the project's 1e-6 relative (README).  Observed worst value over every comparison of this file on an
MI355X: 2.3e-12 (dnorm of the triangular solves against the inverse); against the restated run 4.3e-14."""
import ctypes as C

import numpy as np
import pytest

import l1class_restated as R
from test_gpu_sparse_lasso import _close

pytestmark = pytest.mark.gpu

BOUND = 1e-6
HIST = ("pnorm", "perr", "dnorm", "derr", "objevals")
LOSSES = ("hinge", "sqhinge", "logistic")


def _fits(p, K, losses=None, factor=0.2, **family):
    """K fits on the problem's label columns, lambda = factor * lambda_max of each"""
    fits = []
    for k in range(K):
        f = R.Fit(loss=(losses or ["logistic"] * K)[k], **family)
        f.lam = factor * R.lambda_max(p["D"], p["ELL"][:, k], f)
        fits.append(f)
    return fits


def _device(gpu, p, fits, loop, cols=None, **more):
    cols = list(range(len(fits))) if cols is None else cols
    f0 = fits[cols[0]]
    o = dict(f0.options(), **loop)
    o.update(lossfunction=[fits[k].loss for k in cols], ridge=[fits[k].pen.ridge for k in cols],
             nonnegative=[fits[k].pen.nonnegative for k in cols], z0=np.asfortranarray(p["z0"][:, cols]),
             u0=np.asfortranarray(p["u0"][:, cols]))
    o.update(more)
    return gpu.l1classifier_multi(p["D"], np.asfortranarray(p["ELL"][:, cols]), [fits[k].lam for k in cols], o)


def _restated(p, fits, k, loop):
    return R.run(p["D"], p["ELL"][:, k], fits[k], dict(loop, z0=p["z0"][:, k].copy(), u0=p["u0"][:, k].copy()))


def _compare(got, c, ref, hist=HIST):
    assert int(got["steps"][c]) == ref["steps"], (c, got["steps"][c], ref["steps"])
    k = ref["steps"]
    for key in hist:
        _close(f"{key}[{c}]", got[key][:k, c], np.asarray(ref[key])[:k], BOUND)
    for key in ("xopt", "zopt", "uopt"):
        _close(f"{key}[{c}]", got[key][:, c], ref[key], BOUND)
    if "objevals" in hist:
        _close(f"objopt[{c}]", [got["objopt"][c]], [ref["objopt"]], BOUND)


# ---------------------------------------------------------------------------------------------------- 1. the shapes
@pytest.mark.parametrize("shape, K, iters, what", (
    ((65, 9), 1, 12, "one row past a 64-row block"),
    ((200, 70), 3, 12, "mixed losses: the chunk takes the logistic instantiation"),
    ((300, 449), 2, 12, "one column past every in-register pass's limit"),
    ((100, 130), 2, 12, "m < n"),
    ((16449, 5), 2, 3, "257 row blocks + 1 row: a workgroup of the forward pass takes two row blocks"),
    ((600, 513), 2, 8, "n = 4*128 + 1 = 512 + 1: one past the product's tile edge and the forward pass's LDS panel"),
))
def test_every_iteration_matches_the_restated_run(gpu, shape, K, iters, what):
    p = R.problem(shape, K)
    fits = _fits(p, K, LOSSES[:K] if K == 3 else None)
    loop = dict(maxiters=iters, domaxiters=1, objevals=1, rho=1.5)
    got = _device(gpu, p, fits, loop)
    assert got["xopt"].shape == (shape[1], K) and got["zopt"].shape == (sum(shape), K) == got["uopt"].shape
    assert got["chunk"] == 10 and got["pnorm"].shape == (iters, K)
    for k in range(K):
        _compare(got, k, _restated(p, fits, k, loop))


# ------------------------------------------------------------------------------------------ 2. two chunks, freezing
def test_eleven_fits_duplicate_in_bits_and_a_stopped_fit_is_frozen(gpu):
    shape = (200, 70)
    p = R.problem(shape, 1)
    K = 11
    f = R.Fit(loss="logistic")
    lmax = R.lambda_max(p["D"], p["ELL"][:, 0], f)
    factors = [0.2, 1.25, 0.6, 0.5, 0.1, 0.3, 0.25, 0.8, 0.15, 0.4, 0.2]  # fit 10 = fit 0; fit 1 above lambda_max
    rng = np.random.default_rng(11)
    z0, u0 = (np.asfortranarray(0.1 * rng.standard_normal((sum(shape), K))) for _ in range(2))
    z0[:, 10], u0[:, 10] = z0[:, 0], u0[:, 0]
    o = dict(objevals=1, z0=z0, u0=u0)
    got = gpu.l1classifier_multi(p["D"], p["ELL"], lmax * np.array(factors), o)
    steps = [int(s) for s in got["steps"]]
    print("steps", steps)
    assert max(steps) < 1000 and steps[0] == steps[10]
    for key in ("xopt", "zopt", "uopt") + HIST:
        a, b = np.ascontiguousarray(got[key][:, 0]), np.ascontiguousarray(got[key][:, 10])
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), key
    # the fit above lambda_max stops before the others, with z2 = 0 exactly, and has the bits of the same fit run alone:
    # nothing touched its columns while the others ran on
    assert steps[1] < max(steps) and np.all(got["zopt"][shape[0]:, 1] == 0.0)
    one = gpu.l1classifier_multi(p["D"], p["ELL"], [lmax * factors[1]],
                                 dict(objevals=1, z0=np.asfortranarray(z0[:, 1:2]), u0=np.asfortranarray(u0[:, 1:2])))
    assert int(one["steps"][0]) == steps[1]
    for key in ("xopt", "zopt", "uopt") + HIST:
        a, b = got[key][:, 1], np.ascontiguousarray(one[key][:, 0])
        if key in HIST:
            assert np.isnan(a[steps[1]:]).all()
            a = a[:steps[1]]
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), b.view(np.uint64)), key


# ------------------------------------------------------------------------------------------------------ 3. the family
@pytest.mark.parametrize("member", ("l1weights", "ridge", "nonnegative", "costs"))
def test_the_family(gpu, member):
    shape = (200, 70)
    p = R.problem(shape, 1)
    w = np.linspace(0.5, 2.0, shape[1])
    w[3] = 0.0  # an unpenalised coefficient
    family = dict(l1weights=dict(l1weights=w), ridge=dict(ridge=0.7), nonnegative=dict(nonnegative=1),
                  costs=dict(weights=np.linspace(0.25, 2.0, shape[0]), classcost="balanced"))[member]
    for loss in ("logistic", "sqhinge"):
        fits = _fits(p, 1, [loss], **family)
        loop = dict(maxiters=12, domaxiters=1, objevals=1)
        got = _device(gpu, p, fits, loop)
        _compare(got, 0, _restated(p, fits, 0, loop))
        if member == "nonnegative":
            assert np.all(got["zopt"][shape[0]:, 0] >= 0.0)
        if member == "l1weights":  # weight 0: z = x + u bit for bit
            j = shape[0] + 3
            assert got["zopt"][j, 0] != 0.0


# ---------------------------------------------------------------------------------------- 4. nodualerror, launches
def test_nodualerror_and_the_passes_over_D(gpu):
    shape, K, N = (200, 70), 11, 9
    p = R.problem(shape, K)
    fits = _fits(p, K, [LOSSES[k % 3] for k in range(K)])
    obj = gpu.L1Classifier(p["D"], p["ELL"], [f.lam for f in fits], [f.loss for f in fits])
    try:
        passes = {}
        for nodual in (1, 0):
            loop = dict(maxiters=N, domaxiters=1, objevals=1, nodualerror=nodual)
            summ = obj.run(z0=p["z0"], u0=p["u0"], **loop)
            got = obj.results(summ)
            assert ("dnorm" in got) == (not nodual) and ("derr" in got) == (not nodual)
            passes[nodual] = obj.launches()
            for k in (0, 4, 10):
                ref = _restated(p, fits, k, loop)
                _compare(got, k, ref, ("pnorm", "perr", "objevals") if nodual else HIST)
                if nodual:
                    assert np.isnan(ref["dnorm"]).all()
        # two chunks: per iteration a forward and a transposed pass each, and a transposed pass each before the first;
        # the dual residual adds no launch and no pass over D
        assert passes[1] == passes[0] and passes[0][1] == 2 * (2 * N + 1)
    finally:
        obj.close()


# ------------------------------------------------------------------------------------------ 5. the triangular solves
def test_triangular_solves_take_the_same_steps(gpu):
    p = R.problem((200, 70), 2)
    fits = _fits(p, 2, ["sqhinge", "logistic"])
    loop = dict(objevals=1)
    inv = _device(gpu, p, fits, loop, xsolve="inverse")
    tri = _device(gpu, p, fits, loop, xsolve="trsv")
    assert inv["xsolve"] == "inverse" and tri["xsolve"] == "trsv"
    assert np.array_equal(inv["steps"], tri["steps"]) and int(inv["steps"].max()) < 1000
    for key in ("xopt", "zopt", "uopt") + HIST:
        for k in range(2):
            s = int(inv["steps"][k]) if key in HIST else None
            _close(f"{key}[{k}]", tri[key][:s, k], inv[key][:s, k], BOUND)


# ---------------------------------------------------------------------------------------------- 6. a converged run
def test_a_converged_run_satisfies_the_optimality_conditions_as_the_restated_one(gpu):
    """kkt of the device's z2 within ten times that of the restated run at the same stop (the factor covers the two
    runs stopping one step apart).  Measured: device 1.004e-4, restated 1.004e-4, ratio 1.000, 229 steps both."""
    p = R.problem((400, 120), 1)
    fits = _fits(p, 1)
    got = _device(gpu, p, fits, {})
    ref = _restated(p, fits, 0, {})
    m = 400
    kd = R.kkt(p["D"], p["ELL"][:, 0], fits[0], got["zopt"][m:, 0])
    kr = R.kkt(p["D"], p["ELL"][:, 0], fits[0], ref["zopt"][m:])
    print(f"steps {int(got['steps'][0])} / {ref['steps']}, kkt device {kd:.3e}, restated {kr:.3e}, ratio {kd / kr:.3f}")
    assert abs(int(got["steps"][0]) - ref["steps"]) <= 1 and ref["steps"] < 1000
    assert kd <= 10.0 * kr


# -------------------------------------------------------------------------------------------------------- 7. the path
def test_the_path(gpu):
    """Starts: z0 = 0 and u0 = the multipliers of the all-zero model, rho*u1 = C*ell*phi'(0) = -ell/2 and u2 = -D'u1,
    which are optimal for every lambda >= lambda_max and a plain warm start for the others.  At lambda = lambda_max
    itself the critical coordinate sits ON the soft threshold, and from a cold start a finite ADMM run -- the restated
    one included: 64 steps, one coefficient of 8.0e-4 on this problem -- stops with it just outside; from these starts
    the first point is the all-zero model exactly."""
    shape = (400, 120)
    p = R.problem(shape, 1)
    D, ell = p["D"], p["ELL"][:, 0]
    u1 = -0.5 * ell
    z0 = np.zeros((sum(shape), 10), order="F")
    u0 = np.asfortranarray(np.repeat(np.concatenate([u1, 0.5 * (D.T @ ell)])[:, None], 10, axis=1))
    got = gpu.l1classifier_path(D, ell, 10, dict(z0=z0, u0=u0, objevals=1))
    lams = got["lams"]
    assert lams.size == 10 and lams[0] == pytest.approx(R.lambda_max(D, ell, R.Fit()), rel=1e-14)
    assert lams[-1] == pytest.approx(1e-2 * lams[0], rel=1e-12) and np.all(np.diff(lams) < 0)
    ref_df = []
    for k in range(10):
        r = R.run(D, ell, R.Fit(lam=lams[k]), dict(z0=z0[:, k].copy(), u0=u0[:, k].copy()))
        ref_df.append(int(np.count_nonzero(r["zopt"][shape[0]:])))
    df = [int(v) for v in got["df"]]
    print("df", df, "restated", ref_df)
    assert np.array_equal(got["df"], np.count_nonzero(got["zopt"][shape[0]:], axis=0))
    assert df[0] == 0 and np.all(got["zopt"][shape[0]:, 0] == 0.0) and df[-1] > df[0]
    for k in range(9):
        assert df[k + 1] >= df[k] or ref_df[k + 1] < ref_df[k], (k, df, ref_df)
    for k in range(10):
        one = gpu.l1classifier(D, ell, float(lams[k]), dict(z0=z0[:, k].copy(), u0=u0[:, k].copy(), objevals=1))
        assert one["steps"] == int(got["steps"][k])
        for key in ("xopt", "zopt", "uopt"):
            assert np.array_equal(one[key], got[key][:, k]), (k, key)
        assert one["objopt"] == got["objopt"][k]


def test_the_tester(gpu):
    results, test = gpu.testers.l1classifiertest(seed=1, rows=256, cols=64)
    print({k: test[k] for k in ("objopt", "zeroobj", "accuracy", "df", "steps")})
    assert test["failed"] == 0 and 0 < test["df"] < 64


# --------------------------------------------------------------------------------------------------- 8. the C ABI
def _desc(gpu, p, K, keep):
    L = gpu._lib
    lib = L.load()
    d = L.L1ClassDesc()
    lib.admm_l1class_desc_default(C.byref(d))
    m, n = p["D"].shape
    lam = np.full(K, 0.05)
    keep.extend([lam])
    d.K, d.m, d.n, d.D, d.ldD = K, m, n, L.as_dp(p["D"]), m
    d.ELL, d.nell, d.lam = L.as_dp(p["ELL"]), p["ELL"].shape[1], L.as_dp(lam)
    return lib, d


def _i32(values, keep):
    a = np.ascontiguousarray(values, dtype=np.int32)
    keep.append(a)
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _f64(values, keep):
    a = np.ascontiguousarray(values, dtype=np.float64)
    keep.append(a)
    return a


@pytest.mark.parametrize("name, code, needle", (
    ("K", -1, "K >= 1"), ("loss01", -1, "fit 1: the 0-1 loss"), ("loss_unknown", -1, "fit 2: unknown loss"),
    ("nell", -1, "2 columns"), ("label", -1, "label 5 of column 1"), ("lambda", -1, "fit 2: lambda"),
    ("ridge", -1, "fit 0: ridge"), ("nonneg", -1, "fit 1: nonneg"), ("l1weights", -1, "weight 4"), ("C", -1, "desc.C"),
    ("xsolve", -2, "xsolve"), ("comm", -2, "row-sharded"), ("struct_size", -1, "struct_size"),
))
def test_create_refusals(gpu, name, code, needle):
    L = gpu._lib
    p = R.problem((40, 12), 3)
    keep = []
    lib, d = _desc(gpu, p, 3, keep)
    if name == "K":
        d.K = 0
    elif name == "loss01":
        d.loss = _i32([L.LOSS_HINGE, L.LOSS_01, L.LOSS_LOGISTIC], keep)
    elif name == "loss_unknown":
        d.loss = _i32([L.LOSS_HINGE, L.LOSS_SQHINGE, 4], keep)
    elif name == "nell":
        d.nell = 2
    elif name == "label":
        E = p["ELL"].copy(order="F")
        E[5, 1] = 0.0
        keep.append(E)
        d.ELL = L.as_dp(E)
    elif name == "lambda":
        d.lam = L.as_dp(_f64([0.1, 0.1, -0.1], keep))
    elif name == "ridge":
        d.ridge = L.as_dp(_f64([np.inf, 0.0, 0.0], keep))
    elif name == "nonneg":
        d.nonneg = _i32([0, 2, 0], keep)
    elif name == "l1weights":
        w = np.ones(12)
        w[4] = -1.0
        d.l1weights = L.as_dp(_f64(w, keep))
    elif name == "C":
        d.C = 0.0
    elif name == "xsolve":
        d.xsolve = L.XSOLVE_CG
    elif name == "comm":
        d.comm = C.c_void_p(1)
    elif name == "struct_size":
        d.struct_size += 8
    h = C.c_void_p()
    rc = lib.admm_l1class_create(C.byref(d), C.byref(h))
    msg = lib.admm_last_error().decode()
    assert rc == code and not h.value and msg and needle in msg, (rc, msg)


def test_run_refusals_and_setters(gpu):
    L = gpu._lib
    p = R.problem((40, 12), 3)
    keep = []
    lib, d = _desc(gpu, p, 3, keep)
    h = C.c_void_p()
    L.check(lib.admm_l1class_create(C.byref(d), C.byref(h)))
    try:
        buf = np.zeros(36)
        assert lib.admm_l1class_fetch(h, L.L1C_F_XOPT, L.as_dp(buf), buf.size, None) == -1
        assert "before the first run" in lib.admm_last_error().decode()
        for field, value, code, needle in (("fast", 1, -2, "fast"), ("relax", 1.5, -2, "relaxation"),
                                           ("convtest", 1, -2, "convtest"), ("rho", 0.0, -1, "rho"),
                                           ("struct_size", 4, -1, "struct_size")):
            o = L.L1ClassOptions()
            lib.admm_l1class_options_default(C.byref(o))
            setattr(o, field, value)
            assert lib.admm_l1class_run(h, C.byref(o), None, None) == code, field
            msg = lib.admm_last_error().decode()
            assert msg and needle in msg, (field, msg)
        w = np.ones(40)
        w[7] = -1.0
        assert lib.admm_l1class_set_cost(h, L.as_dp(w), None) == -1 and lib.admm_last_error().decode()
        lw = np.ones(12)
        lw[2] = np.nan
        assert lib.admm_l1class_set_l1weights(h, L.as_dp(lw)) == -1 and "weight 2" in lib.admm_last_error().decode()
        a = C.c_int64(0)
        assert lib.admm_l1class_launches(h, C.byref(a), None) == -1 and lib.admm_last_error().decode()
    finally:
        lib.admm_l1class_destroy(h)


def test_a_bare_abi_sequence_runs_twice_with_another_rho(gpu):
    """create, run (rho = 1), run again on the same object with rho = 2.5 -- the factor does not depend on rho --, fetch:
    the second run against the restated run at rho = 2.5"""
    L = gpu._lib
    shape, K, N = (100, 130), 2, 10
    p = R.problem(shape, K)
    keep = []
    lib, d = _desc(gpu, p, K, keep)
    d.loss = _i32([L.LOSS_SQHINGE, L.LOSS_LOGISTIC], keep)
    h = C.c_void_p()
    L.check(lib.admm_l1class_create(C.byref(d), C.byref(h)))
    try:
        summ = (L.L1ClassSummary * K)()
        for rho in (1.0, 2.5):
            o = L.L1ClassOptions()
            lib.admm_l1class_options_default(C.byref(o))
            o.maxiters, o.domaxiters, o.objevals, o.rho = N, 1, 1, rho
            o.z0, o.u0 = L.as_dp(p["z0"]), L.as_dp(p["u0"])
            rt = C.c_double(0)
            L.check(lib.admm_l1class_run(h, C.byref(o), summ, C.byref(rt)))
            assert [s.steps for s in summ] == [N, N] and rt.value > 0
        got = {}
        for key, field, rows in (("xopt", L.L1C_F_XOPT, shape[1]), ("zopt", L.L1C_F_ZOPT, sum(shape)),
                                 ("uopt", L.L1C_F_UOPT, sum(shape)), ("pnorm", L.L1C_F_PNORM, N),
                                 ("dnorm", L.L1C_F_DNORM, N), ("objevals", L.L1C_F_OBJEVALS, N)):
            buf = np.empty((rows, K), order="F")
            wr = C.c_size_t(0)
            L.check(lib.admm_l1class_fetch(h, field, L.as_dp(buf), buf.size, C.byref(wr)))
            assert wr.value == buf.size
            got[key] = buf
        small = np.empty(3)
        assert lib.admm_l1class_fetch(h, L.L1C_F_ZOPT, L.as_dp(small), small.size, None) == -6
        for k, loss in enumerate(("sqhinge", "logistic")):
            ref = R.run(p["D"], p["ELL"][:, k], R.Fit(loss=loss, lam=0.05),
                        dict(maxiters=N, domaxiters=1, objevals=1, rho=2.5, z0=p["z0"][:, k].copy(), u0=p["u0"][:, k].copy()))
            for key in ("pnorm", "dnorm", "objevals"):
                _close(f"{key}[{k}]", got[key][:, k], np.asarray(ref[key]), BOUND)
            for key in ("xopt", "zopt", "uopt"):
                _close(f"{key}[{k}]", got[key][:, k], ref[key], BOUND)
    finally:
        lib.admm_l1class_destroy(h)
