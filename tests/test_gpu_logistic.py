"""lossfunction = 'logistic' on the device: one element update against long double, full runs of every iteration form
against the restated oracle (tests/logistic_restated.py), one-vs-rest columns mixed with the other losses, the C ABI's
loss values and the MEX gateway.  1e-7 is the single-class path's own tolerance (test_svm_hinge, as quoted in
tests/test_gpu_svm_ovr.py)."""
import ctypes as C

import numpy as np
import pytest

import logistic_restated as R
from oracle import solvers_ref as S

pytestmark = pytest.mark.gpu

PLAIN = ("xvals", "zvals", "uvals", "pnorm", "perr", "objevals", "Hnormsq")  # (nodualerror: dnorm, derr are NaN)
STRONG = PLAIN + ("vvals", "uhatvals", "avals")
WEAK = ("xvals", "zvals", "uvals", "vvals", "uhatvals", "objevals", "Hnormsq", "avals", "dvals", "restarted")
OVR_HIST = ("pnorm", "perr", "Hnormsq", "objevals")


def _err(name, got, ref, tol=1e-7):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert not np.isnan(got).any() and not np.isnan(ref).any(), f"{name}: NaN"
    err = float(np.max(np.abs(got - ref)) / max(1e-300, np.max(np.abs(ref))))
    print(f"{name}: relative error {err:.3e} (bound {tol:g})")
    assert err < tol, f"{name}: relative error {err:.3e} >= {tol:g}"


def _same_run(got, ref, steps=None, hist=PLAIN):
    """every history of the case (a missing one is a failure), the final iterates, the objective and the step count"""
    assert int(got["steps"]) == int(ref["steps"]), (got["steps"], ref["steps"])
    if steps is not None:
        assert int(got["steps"]) == steps
    for key in hist:
        assert key in got and key in ref, key
        _err(key, got[key], ref[key])
    for key in ("xopt", "zopt", "uopt"):
        _err(key, got[key], ref[key])
    _err("objopt", [got["objopt"]], [ref["objopt"]])


def _device_loop(gpu, D, ell, Cv, o, maxiters):
    """a forced run shorter than unwrappedadmm.m:90's 1000: the loop entered through admm() with the library operators"""
    from admm_project_amd.solvers import _ENGINE_OBJ
    m = D.shape[0]
    gx, gz, _ = gpu.getproxops("LinearSVM", dict(D=D, ell=ell, C=Cv, lossfunction="logistic"))
    return gpu.admm(gx, gz, dict(o, A=D, At=D.T, B=-1, nB=m, c=0, m=m, maxiters=maxiters, stopcond="both", nodualerror=1,
                                 obj=_ENGINE_OBJ))


# ------------------------------------------------------------------------------------------- one element update
@pytest.fixture(scope="module")
def yardstick():
    """the restatement's own error against long double, in units of eps*(|w| + t + 1) (test_logistic_host)"""
    gw, gt = R.grid_pairs()
    rw, rt = R.random_pairs()
    w, t = np.concatenate([gw, rw]), np.concatenate([gt, rt])
    r = float(R.ratio(R.prox_root(w, t), R.prox_root(w, t, np.longdouble), w, t).max())
    print(f"restatement ratio {r:.3f}")
    return r


@pytest.mark.parametrize("C_rho", [(0.0, 1.0), (1e-12, 1.0), (0.5, 0.5), (1e3, 1e-3)], ids=["t=0", "t=1e-12", "t=1", "t=1e6"])
@pytest.mark.parametrize("shape", [(37, 5), (129, 8)])
def test_one_element_update_against_long_double(gpu, yardstick, shape, C_rho):
    """D = the first n columns of I_m: x = (z0 - u0)[:n], so D*x + u0 = v is the test's choice (z0 = v, u0 = 0 on the
    first n rows; u0 = v below).  One iteration (the two-launch form: uw_prox_kernel<true>).  Measured on the device:
    max ratio 0.41 (t = 1e-12), 0.40 (t = 1), below 0.001 (t = 1e6), 0 (t = 0) against the restatement's 0.99"""
    m, n = shape
    Cv, rho = C_rho
    t = Cv / rho
    rng = np.random.default_rng(m)
    grid = np.array(R.GRID_W)
    w = np.concatenate([grid, grid, rng.uniform(-50, 50, m - 2 * grid.size)])
    ell = np.concatenate([np.ones(grid.size), -np.ones(grid.size), np.where(rng.random(m - 2 * grid.size) < 0.5, 1.0, -1.0)])
    perm = rng.permutation(m)
    v, ell = (ell * w)[perm], ell[perm]
    D = np.asfortranarray(np.eye(m, n))
    z0, u0 = np.zeros(m), v.copy()
    z0[:n], u0[:n] = v[:n], 0.0
    got = _device_loop(gpu, D, ell, Cv, dict(rho=rho, domaxiters=1, objevals=1, x0=np.zeros(n), z0=z0, u0=u0), 1)
    assert int(got["steps"]) == 1
    x = np.asarray(got["xopt"])
    assert np.allclose(x, v[:n], rtol=4 * R.EPS, atol=0.0)  # I'I = I
    v = v.copy()
    v[:n] = x  # D*x + u0 as the device formed it: x itself on the first n rows (u0 = 0 there), u0 below
    z = np.asarray(got["zopt"])
    assert np.isfinite(z).all()
    z_ld = R.prox(v, ell, t, np.longdouble)
    ratio = R.ratio(z, z_ld, v, t)
    print(f"m x n = {m} x {n}, t = {t:g}: device max |z - z_ld| / (eps*(|v| + t + 1)) = {ratio.max():.3f} "
          f"(restatement {yardstick:.3f})")
    assert ratio.max() <= max(8.0, 4.0 * yardstick)
    if t == 0.0:
        assert np.array_equal(z, v)  # bit for bit
    Dx = np.concatenate([x, np.zeros(m - n)]).astype(np.longdouble)
    obj_ld = np.longdouble(0.5) * np.sum(Dx * Dx) + np.longdouble(Cv) * np.sum(np.logaddexp(np.longdouble(0), -ell * Dx))
    obj = float(got["objevals"][0])
    assert np.isfinite(obj)
    rel = abs(obj - float(obj_ld)) / abs(float(obj_ld))
    print(f"objective {obj!r} against long double {float(obj_ld)!r}: relative {rel:.3e}")
    assert rel <= 1e-12


# ---------------------------------------------------------------------------------- full runs, every iteration form
@pytest.fixture(scope="module")
def problems(ap):
    labels = ap.synth.reference_mnist_labels("train")
    out = {"256x2": ap.synth.svm_problem(0), "700x57": ap.synth.mnist_like_problem(seed=1, m=700, n=57, labels=labels),
           "600x449": ap.synth.mnist_like_problem(seed=2, m=600, n=449),
           "16385x8": ap.synth.mnist_like_problem(seed=3, m=16385, n=8)}
    return out


@pytest.fixture(scope="module")
def refs(problems):
    """restated oracle runs, each computed once"""
    cache = {}

    def get(name, maxiters=None, workers=1, **o):
        key = (name, maxiters, workers, tuple(sorted(o.items())))
        if key not in cache:
            p = problems[name]
            cache[key] = R.run(p["D"], p["ell"], p["C"], dict(o, objevals=1, x0=p["x0"], z0=p["z0"], u0=p["u0"]),
                               workers=workers, maxiters=maxiters)
        return cache[key]
    return get


@pytest.mark.parametrize("name", ["256x2", "700x57"])
def test_small_problems_run_to_their_stop(gpu, problems, refs, name):
    """below 48 MiB of D the engine takes the two-launch form (uw_ax_kernel + uw_prox_kernel) whatever n is.  On a build
    without the loss 'logistic' trains a hinge SVM: this fails there"""
    p = problems[name]
    ref = refs(name)
    assert 20 <= ref["steps"] <= 30
    got = gpu.linearsvm(p["D"], p["ell"], p["C"], dict(lossfunction="logistic", objevals=1, x0=p["x0"], z0=p["z0"],
                                                        u0=p["u0"]))
    _same_run(got, ref)


@pytest.mark.parametrize("name,iters", [("600x449", 30), ("16385x8", 20)])
def test_forced_runs_two_launches_and_many_row_blocks(gpu, problems, refs, name, iters):
    """the two-launch form: n = 449, the first width past the one-pass kernel's limit, and m = 16385, where a workgroup
    of uw_prox_kernel takes several row blocks"""
    p = problems[name]
    ref = refs(name, maxiters=iters, domaxiters=1)
    got = _device_loop(gpu, p["D"], p["ell"], p["C"], dict(domaxiters=1, objevals=1, x0=p["x0"], z0=p["z0"], u0=p["u0"]),
                       iters)
    _same_run(got, ref, steps=iters)


def test_one_pass_form(gpu, ap, monkeypatch):
    """ad_onepass_kernel<true>: 14081 x 448 is 48.1 MiB of D (onepass_supported: n <= 448 and at least 48 MiB), the widest
    D and a ragged last block of one row; 12 forced iterations against the restated oracle, against the two-launch form of
    the same engine (ADMM_HIP_NO_ONEPASS) and, as test_one_pass_iteration_on_a_tall_narrow_matrix shows it, that the
    one-pass form is what ran (no D*x launch of its own)"""
    m, n, iters = 14081, 448, 12
    assert m * n * 8 >= 48 << 20
    p = ap.synth.mnist_like_problem(seed=4, m=m, n=n, labels=ap.synth.reference_mnist_labels("train"))
    o = dict(domaxiters=1, objevals=1, x0=p["x0"], z0=p["z0"], u0=p["u0"])
    ref = R.run(p["D"], p["ell"], p["C"], o, maxiters=iters)
    got = _device_loop(gpu, p["D"], p["ell"], p["C"], o, iters)
    monkeypatch.setenv("ADMM_HIP_NO_ONEPASS", "1")
    gen = _device_loop(gpu, p["D"], p["ell"], p["C"], o, iters)
    monkeypatch.delenv("ADMM_HIP_NO_ONEPASS")
    _same_run(got, ref, steps=iters)
    for key in PLAIN + ("xopt", "zopt", "uopt"):
        _err(f"{key} (one pass against two launches)", got[key], gen[key], 1e-9)
    L = gpu._lib
    eng = gpu.Engine(L.PROB_LINEARSVM, D=p["D"], ell=p["ell"], Cval=p["C"], loss=L.LOSS_LOGISTIC)
    try:
        eng.set_profiling([L.K_GEMV_N, L.K_PROX])
        eng.run(maxiters=5, domaxiters=1, record_history=0, nodualerror=1)
        assert eng.kernel_time(L.K_GEMV_N)[1] == 0 and eng.kernel_time(L.K_PROX)[1] == 5
    finally:
        eng.close()


@pytest.mark.parametrize("fasttype", ["strong", "weak"])
def test_fast_admm(gpu, problems, refs, fasttype):
    """ADMM_FAST_STRONG = 1 and ADMM_FAST_WEAK = 2 (the restarted form)"""
    p = problems["256x2"]
    ref = refs("256x2", fast=1, fasttype=fasttype)
    got = gpu.linearsvm(p["D"], p["ell"], p["C"], dict(lossfunction="logistic", fast=1, fasttype=fasttype, objevals=1,
                                                        x0=p["x0"], z0=p["z0"], u0=p["u0"]))
    _same_run(got, ref, hist=STRONG if fasttype == "strong" else WEAK)


def test_three_workers(gpu, problems, refs):
    """parallel = 'both': the transpose-reduction x-update and the sliced z-prox (the generic prox kernel)"""
    p = problems["256x2"]
    ref = refs("256x2", workers=3, parallel="both")
    got = gpu.linearsvm(p["D"], p["ell"], p["C"], dict(lossfunction="logistic", parallel="both", workers=3, objevals=1,
                                                        x0=p["x0"], z0=p["z0"], u0=p["u0"]))
    _same_run(got, ref)


# ------------------------------------------------------------------------------------------------- one-vs-rest
def _starts(rng, n, m, K):
    x0, z0, u0 = np.empty((n, K), order="F"), np.empty((m, K), order="F"), np.empty((m, K), order="F")
    for c in range(K):
        x0[:, c], z0[:, c], u0[:, c] = rng.random(n), rng.random(m), rng.random(m)
    return x0, z0, u0


def _compare_class(got, c, ref, limit=None):
    k = int(got["steps"][c]) if limit is None else limit
    for key in OVR_HIST:
        _err(f"{key}[{c}]", got[key][:k, c], np.asarray(ref[key])[:k])
    if limit is None:
        assert int(got["steps"][c]) == int(ref["steps"])
        for key in OVR_HIST:
            assert np.isnan(got[key][k:, c]).all()  # NaN past the class's last step
        for key in ("xopt", "zopt", "uopt"):
            _err(f"{key}[{c}]", got[key][:, c], ref[key])
        _err(f"objopt[{c}]", [got["objopt"][c]], [ref["objopt"]])


def test_ovr_twelve_columns_two_passes(gpu, problems):
    """classes 0..9 logistic, then class 0 hinge and class 1 with '01': 10 + 2 columns, the second pass mixes losses
    with no logistic class in it, the first is all logistic"""
    p = problems["700x57"]
    D, Cv = p["D"], p["C"]
    lab = np.asarray(gpu.synth.reference_mnist_labels("train")[:700], dtype=np.float64)
    classes = np.concatenate([np.arange(10.0), [0.0, 1.0]])
    losses = ["logistic"] * 10 + ["hinge", "01"]
    x0, z0, u0 = _starts(np.random.default_rng(7), 57, 700, 12)
    got = gpu.linearsvm_ovr(D, lab, Cv, dict(objevals=1, classes=classes, lossfunction=losses, x0=x0, z0=z0, u0=u0))
    steps = []
    for c in range(10):
        ell = np.where(lab == c, 1.0, -1.0)
        ref = R.run(D, ell, Cv, dict(objevals=1, x0=x0[:, c], z0=z0[:, c], u0=u0[:, c]))
        steps.append(ref["steps"])
        _compare_class(got, c, ref)
    print("logistic steps per class:", steps)
    assert len(set(steps)) > 1  # they freeze at different times
    ref = S.linearsvm(D, np.where(lab == 0, 1.0, -1.0), Cv, dict(objevals=1, x0=x0[:, 10], z0=z0[:, 10], u0=u0[:, 10]))
    _compare_class(got, 10, ref)  # unaffected by its neighbours
    k = int(got["steps"][11])
    assert 1 <= k <= 1000
    for key in ("xopt", "zopt", "uopt"):
        assert np.isfinite(got[key][:, 11]).all()
    for key in OVR_HIST:
        assert np.isfinite(got[key][:k, 11]).all()
    assert np.isfinite(got["objopt"][11])


def test_ovr_mixed_chunk_many_row_blocks(gpu, problems, refs):
    """16385 x 8, columns logistic, hinge, logistic in one chunk, 20 forced iterations: the multi-block pass"""
    p = problems["16385x8"]
    D, ell, Cv = p["D"], p["ell"], p["C"]
    m, n = D.shape
    ELL = np.asfortranarray(np.stack([ell, ell, -ell], axis=1))
    x0, z0, u0 = (np.asfortranarray(np.stack([p[k], p[k], p[k]], axis=1)) for k in ("x0", "z0", "u0"))
    L = gpu._lib
    obj = gpu.SvmOvr(D, ELL, Cv, ["logistic", "hinge", "logistic"])
    try:
        summ = obj.run(maxiters=20, domaxiters=1, objevals=1, x0=x0, z0=z0, u0=u0)
        got = dict(steps=summ["steps"], objopt=summ["objopt"], xopt=obj.fetch(L.OVR_F_XOPT, n), zopt=obj.fetch(L.OVR_F_ZOPT, m),
                   uopt=obj.fetch(L.OVR_F_UOPT, m), pnorm=obj.fetch(L.OVR_F_PNORM, 20), perr=obj.fetch(L.OVR_F_PERR, 20),
                   Hnormsq=obj.fetch(L.OVR_F_HNORMSQ, 20), objevals=obj.fetch(L.OVR_F_OBJEVALS, 20))
    finally:
        obj.close()
    assert list(got["steps"]) == [20, 20, 20]
    o = dict(objevals=1, domaxiters=1, x0=p["x0"], z0=p["z0"], u0=p["u0"])
    for c, ref in ((0, refs("16385x8", maxiters=20, domaxiters=1)), (2, R.run(D, -ell, Cv, o, maxiters=20))):
        _compare_class(got, c, ref, limit=20)
        for key in ("xopt", "zopt", "uopt"):
            _err(f"{key}[{c}]", got[key][:, c], ref[key])
        _err(f"objopt[{c}]", [got["objopt"][c]], [ref["objopt"]])
    ref = S.linearsvm(D, ell, Cv, o)
    _compare_class(got, 1, ref, limit=20)
    for key, hist in (("xopt", "xvals"), ("zopt", "zvals"), ("uopt", "uvals")):
        _err(f"{key}[1]", got[key][:, 1], ref[hist][:, 19])


# ------------------------------------------------------------------------------------------ C ABI and MEX gateway
def test_c_abi_loss_values(gpu, ap):
    L = ap._lib
    lib = L.load()
    rng = np.random.default_rng(0)
    D = np.asfortranarray(rng.random((64, 4)))
    E = np.asfortranarray(np.where(rng.random((64, 2)) < 0.5, 1.0, -1.0))
    for values, code in (((3, 4), L.E_INVALID), ((-1, 0), L.E_INVALID), ((3, 1), L.OK), ((2, 3), L.OK)):
        loss = np.ascontiguousarray(values, dtype=np.int32)
        d = L.SvmOvrDesc()
        lib.admm_svm_ovr_desc_default(C.byref(d))
        d.K, d.m, d.n, d.D, d.ldD, d.C, d.ELL = 2, 64, 4, L.as_dp(D), 64, 0.5, L.as_dp(E)
        d.loss = loss.ctypes.data_as(C.POINTER(C.c_int32))
        h = C.c_void_p()
        rc = lib.admm_svm_ovr_create(C.byref(d), C.byref(h))
        assert rc == code, (values, rc)
        if code == L.OK:
            lib.admm_svm_ovr_destroy(h)
        else:
            assert not h.value and b"bad loss for class" in lib.admm_last_error()


def test_mex_gateway_logistic(gpu, problems, tmp_path_factory):
    """as test_mex_gateway's LinearSVM case: args.lossfunction = 'logistic' reaches the binding unchanged"""
    from mexharness import Harness, build
    mex = Harness(build(tmp_path_factory.mktemp("mexlog")))
    p = problems["256x2"]
    D, ell, Cv = p["D"], p["ell"], p["C"]
    m = D.shape[0]
    args = dict(D=D, Dt=D.T, ell=ell, C=Cv, lossfunction="logistic")
    options = dict(objevals=1, A=D, At=D.T, B=-1, nB=m, c=0, m=m, x0=p["x0"], z0=p["z0"], u0=p["u0"], maxiters=1000,
                   stopcond="both", nodualerror=1)
    got = mex.call("solve", "linearsvm", args, options, dict(objnative=1))
    ref = gpu.linearsvm(D, ell, Cv, dict(lossfunction="logistic", objevals=1, x0=p["x0"], z0=p["z0"], u0=p["u0"]))
    assert int(got["steps"]) == int(ref["steps"])
    _err("xopt", got["xopt"], ref["xopt"], 1e-12)
    _err("objevals", got["objevals"], ref["objevals"], 1e-12)
