"""Per-observation costs, class costs and the squared hinge of the linear SVM on the device: the element update
(admm_op_svm_prox) against long double, full runs of every iteration form against the restated oracle
(tests/svm_cost_restated.py), the one-vs-rest pass with shared weights and per-class costs, the defaults, the C ABI's
refusals and the MEX gateway.  1e-7 is the single-class path's own tolerance (test_svm_hinge, as quoted in
tests/test_gpu_svm_ovr.py)."""
import ctypes as C

import numpy as np
import pytest

import svm_cost_restated as R
from oracle import solvers_ref as S

pytestmark = pytest.mark.gpu

PLAIN = ("xvals", "zvals", "uvals", "pnorm", "perr", "objevals", "Hnormsq")  # (nodualerror: dnorm, derr are NaN)
STRONG = PLAIN + ("vvals", "uhatvals", "avals")
WEAK = ("xvals", "zvals", "uvals", "vvals", "uhatvals", "objevals", "Hnormsq", "avals", "dvals", "restarted")
OVR_HIST = ("pnorm", "perr", "Hnormsq", "objevals")
COSTS = (5.07, 0.55)
LD = np.longdouble


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


def _weights(m, seed):
    w = np.random.default_rng(seed).uniform(0.25, 4.0, m)
    w[::17] = 0.0
    return w


def _device_loop(gpu, D, ell, Cv, loss, cost_args, o, maxiters):
    """a forced run shorter than unwrappedadmm.m:90's 1000: the loop entered through admm() with the library operators"""
    from admm_project_amd.solvers import _ENGINE_OBJ
    m = D.shape[0]
    gx, gz, _ = gpu.getproxops("LinearSVM", dict(D=D, ell=ell, C=Cv, lossfunction=loss, **cost_args))
    return gpu.admm(gx, gz, dict(o, A=D, At=D.T, B=-1, nB=m, c=0, m=m, maxiters=maxiters, stopcond="both", nodualerror=1,
                                 obj=_ENGINE_OBJ))


# ------------------------------------------------------------------------------------------- one element update
LOSS_CODE = {"hinge": 0, "01": 1, "logistic": 3, "sqhinge": 5}


def _op(ap, v, ell, loss, Cv, rho, w, costs):
    L = ap._lib
    out = np.empty_like(v)
    wv = None if w is None else np.ascontiguousarray(w)
    d = L.SvmCostDesc(None if wv is None else L.as_dp(wv), costs[0], costs[1])
    L.check(L.load().admm_op_svm_prox(L.as_dp(v), L.as_dp(ell), v.size, LOSS_CODE[loss], Cv, rho, C.byref(d), L.as_dp(out)))
    return out


@pytest.mark.parametrize("loss", R.LOSSES)
def test_one_element_update_against_long_double(gpu, ap, loss):
    """admm_op_svm_prox runs svm_cost_prox_elem, the loop's own device function, on lengths 1, 63, 64, 65, 129 and 1000
    with weights whose every 17th value is 0, costs (5.07, 0.55) and t = C/rho in {0, 1e-12, 1, 1e6}; s on and one ulp
    beside the kinks 1, 1 - t_i, 1 + 2 t_i, plus random v ('01': constructed at least 1e-6 away from its two
    thresholds).  Bound: max(8, 4 r)*eps*(|v| + t_i + 1) with r the restatement's own ratio on the same inputs.
    Measured on the device (max ratio; restatement): hinge 0.339 (0.339), sqhinge 0.773 (0.773), logistic 0.339 (0.839),
    '01' 0 (0); rows with c_i = 0 return v bit for bit"""
    worst = rworst = 0.0
    for length in (1, 63, 64, 65, 129, 1000):
        for t in R.GRID_T:
            make = R.element_inputs_01 if loss == "01" else R.element_inputs
            v, ell, w = make(length, t, COSTS, 100 * length + int(np.log10(t + 1e-13)))
            ci = w * np.where(ell > 0, COSTS[0], COSTS[1])
            ti = t * ci  # = (C*c_i)/rho with C = t, rho = 1
            z = _op(ap, v, ell, loss, t, 1.0, w, COSTS)
            assert np.isfinite(z).all()
            z_ld = R.prox(v, ell, ti, loss, LD)
            r = float(R.ratio(R.prox(v, ell, ti, loss), z_ld, v, ti).max())
            ratio = R.ratio(z, z_ld, v, ti)
            worst, rworst = max(worst, float(ratio.max())), max(rworst, r)
            assert ratio.max() <= max(8.0, 4.0 * r), (loss, length, t, float(ratio.max()), r)
            zero = ci == 0.0
            assert zero[0] and np.array_equal(z[zero], v[zero])  # bit for bit
            if t == 0.0:
                assert np.array_equal(z, v)
    print(f"{loss}: device max |z - z_ld| / (eps*(|v| + t_i + 1)) = {worst:.3f} (restatement {rworst:.3f})")


def test_element_update_defaults_and_refusals(gpu, ap):
    """desc == NULL is unit costs: the hinge prox of the oracle; the refusals are admm_engine_set_svm_cost's"""
    L = ap._lib
    lib = L.load()
    rng = np.random.default_rng(0)
    v, ell = rng.uniform(-3, 3, 130), np.where(rng.random(130) < 0.5, 1.0, -1.0)
    out = np.empty_like(v)
    L.check(lib.admm_op_svm_prox(L.as_dp(v), L.as_dp(ell), v.size, 0, 0.5, 2.0, None, L.as_dp(out)))
    assert np.array_equal(out, R.prox(v, ell, 0.25, "hinge"))
    for loss, w, costs in ((4, None, (1.0, 1.0)), (6, None, (1.0, 1.0)), (0, -np.ones(130), (1.0, 1.0)),
                           (0, None, (np.nan, 1.0)), (5, None, (1.0, -1.0))):
        d = L.SvmCostDesc(None if w is None else L.as_dp(w), costs[0], costs[1])
        assert lib.admm_op_svm_prox(L.as_dp(v), L.as_dp(ell), v.size, loss, 0.5, 2.0, C.byref(d), L.as_dp(out)) == L.E_INVALID


# ---------------------------------------------------------------------------------- full runs, every iteration form
@pytest.fixture(scope="module")
def problems(ap):
    labels = ap.synth.reference_mnist_labels("train")
    out = {"256x2": ap.synth.svm_problem(0), "700x57": ap.synth.mnist_like_problem(seed=1, m=700, n=57, labels=labels),
           "600x449": ap.synth.mnist_like_problem(seed=2, m=600, n=449),
           "16385x8": ap.synth.mnist_like_problem(seed=3, m=16385, n=8)}
    for k, p in enumerate(out.values()):
        p["w"] = _weights(p["ell"].size, 20 + k)
        p["cost"] = R.cost_vector(p["ell"], p["w"], "balanced")
    return out


@pytest.fixture(scope="module")
def refs(problems):
    """restated oracle runs with weights and 'balanced' class costs, each computed once"""
    cache = {}

    def get(name, loss, maxiters=None, workers=1, **o):
        key = (name, loss, maxiters, workers, tuple(sorted(o.items())))
        if key not in cache:
            p = problems[name]
            cache[key] = R.run(p["D"], p["ell"], p["C"], p["cost"], loss,
                               dict(o, objevals=1, x0=p["x0"], z0=p["z0"], u0=p["u0"]), workers=workers, maxiters=maxiters)
        return cache[key]
    return get


def _opts(p, loss, **more):
    return dict(more, lossfunction=loss, weights=p["w"], classcost="balanced", objevals=1, x0=p["x0"], z0=p["z0"], u0=p["u0"])


PLAIN_STEPS = {"256x2": 38, "700x57": 73}  # the plain hinge SVM (test_svm_cost_host)


@pytest.mark.parametrize("loss", ["hinge", "sqhinge"])
@pytest.mark.parametrize("name", ["256x2", "700x57"])
def test_small_problems_run_to_their_stop(gpu, problems, refs, name, loss):
    """below 48 MiB of D the engine takes the two-launch form (uw_ax_kernel + uw_prox_kernel<., SvmCostArgs>).  On a
    build without the feature the options are ignored and a plain hinge SVM is trained (38 / 73 steps): this fails there.
    With these weights the restatement stops after 76 / 49 steps (256 x 2: hinge / sqhinge) and 125 / 62 (700 x 57)"""
    p = problems[name]
    ref = refs(name, loss)
    print(f"{name} {loss}: the restatement stops after {ref['steps']} steps")
    assert ref["steps"] < 1000 and ref["steps"] != PLAIN_STEPS[name]
    got = gpu.linearsvm(p["D"], p["ell"], p["C"], _opts(p, loss))
    _same_run(got, ref)


@pytest.mark.parametrize("name,iters", [("600x449", 30), ("16385x8", 20)])
def test_forced_runs_two_launches_and_many_row_blocks(gpu, problems, refs, name, iters):
    """the two-launch form: n = 449, the first width past the one-pass kernel's limit, and m = 16385, where a workgroup
    of uw_prox_kernel takes several row blocks; 'sqhinge' with costs"""
    p = problems[name]
    ref = refs(name, "sqhinge", maxiters=iters, domaxiters=1)
    got = _device_loop(gpu, p["D"], p["ell"], p["C"], "sqhinge", dict(weights=p["w"], classcost="balanced"),
                       dict(domaxiters=1, objevals=1, x0=p["x0"], z0=p["z0"], u0=p["u0"]), iters)
    _same_run(got, ref, steps=iters)


def test_one_pass_form(gpu, ap, monkeypatch):
    """ad_onepass_kernel<false, SvmCostArgs>: 14081 x 448 is 48.1 MiB of D (onepass_supported: n <= 448 and at least
    48 MiB), the widest D and a ragged last block of one row; hinge with costs, 12 forced iterations against the restated
    oracle, against the two-launch form of the same engine (ADMM_HIP_NO_ONEPASS) and, as test_one_pass_form of
    test_gpu_logistic shows it, that the one-pass form is what ran (no D*x launch of its own)"""
    m, n, iters = 14081, 448, 12
    assert m * n * 8 >= 48 << 20
    p = ap.synth.mnist_like_problem(seed=4, m=m, n=n, labels=ap.synth.reference_mnist_labels("train"))
    w = _weights(m, 31)
    cost = R.cost_vector(p["ell"], w, COSTS)
    o = dict(domaxiters=1, objevals=1, x0=p["x0"], z0=p["z0"], u0=p["u0"])
    ca = dict(weights=w, classcost=COSTS)
    ref = R.run(p["D"], p["ell"], p["C"], cost, "hinge", o, maxiters=iters)
    got = _device_loop(gpu, p["D"], p["ell"], p["C"], "hinge", ca, o, iters)
    monkeypatch.setenv("ADMM_HIP_NO_ONEPASS", "1")
    gen = _device_loop(gpu, p["D"], p["ell"], p["C"], "hinge", ca, o, iters)
    monkeypatch.delenv("ADMM_HIP_NO_ONEPASS")
    _same_run(got, ref, steps=iters)
    for key in PLAIN + ("xopt", "zopt", "uopt"):
        _err(f"{key} (one pass against two launches)", got[key], gen[key], 1e-9)
    L = gpu._lib
    eng = gpu.Engine(L.PROB_LINEARSVM, D=p["D"], ell=p["ell"], Cval=p["C"], loss=L.LOSS_HINGE)
    try:
        eng.set_svm_cost(w, COSTS)
        eng.set_profiling([L.K_GEMV_N, L.K_PROX])
        eng.run(maxiters=5, domaxiters=1, record_history=0, nodualerror=1)
        assert eng.kernel_time(L.K_GEMV_N)[1] == 0 and eng.kernel_time(L.K_PROX)[1] == 5
    finally:
        eng.close()


@pytest.mark.parametrize("loss", ["hinge", "sqhinge"])
@pytest.mark.parametrize("fasttype", ["strong", "weak"])
def test_fast_admm(gpu, problems, refs, fasttype, loss):
    """ADMM_FAST_STRONG = 1 and ADMM_FAST_WEAK = 2 (the restarted form): the generic prox kernels with costs"""
    p = problems["256x2"]
    ref = refs("256x2", loss, fast=1, fasttype=fasttype)
    got = gpu.linearsvm(p["D"], p["ell"], p["C"], _opts(p, loss, fast=1, fasttype=fasttype))
    _same_run(got, ref, hist=STRONG if fasttype == "strong" else WEAK)


@pytest.mark.parametrize("loss", ["hinge", "sqhinge"])
def test_three_workers(gpu, problems, refs, loss):
    """parallel = 'both': the transpose-reduction x-update and the sliced z-prox (the generic prox kernel)"""
    p = problems["256x2"]
    ref = refs("256x2", loss, workers=3, parallel="both")
    got = gpu.linearsvm(p["D"], p["ell"], p["C"], _opts(p, loss, parallel="both", workers=3))
    _same_run(got, ref)


def test_logistic_and_01_with_costs(gpu, problems, refs):
    """the other two losses through the cost form of the two-launch kernel (uw_prox_kernel<true, SvmCostArgs> for the
    logistic one); the 0-1 run is discontinuous in its data, so it is held to its step count and finite results, as
    test_gpu_logistic holds its '01' column"""
    p = problems["700x57"]
    _same_run(gpu.linearsvm(p["D"], p["ell"], p["C"], _opts(p, "logistic")), refs("700x57", "logistic"))
    got = gpu.linearsvm(p["D"], p["ell"], p["C"], _opts(p, "01"))
    assert 1 <= int(got["steps"]) <= 1000 and np.isfinite(got["xopt"]).all() and np.isfinite(got["objopt"])


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
    """700 x 57: classes 0..9 'balanced', alternating 'sqhinge' and hinge, then class 0 logistic with costs (5.07, 0.55)
    and class 1 hinge with costs (1, 1): 10 + 2 columns, two passes.  First with weights shared by all classes (every
    column against its own restated run); then the same classes without weights, where the last column has unit cost
    inside a chunk that runs the cost form: against the oracle's own hinge SVM"""
    p = problems["700x57"]
    D, Cv, w = p["D"], p["C"], p["w"]
    lab = np.asarray(gpu.synth.reference_mnist_labels("train")[:700], dtype=np.float64)
    classes = np.concatenate([np.arange(10.0), [0.0, 1.0]])
    losses = ["sqhinge", "hinge"] * 5 + ["logistic", "hinge"]
    ELL = np.where(lab[:, None] == classes[None, :], 1.0, -1.0)
    pos = np.sum(ELL[:, :10] > 0, axis=0)
    cc = np.array([[700 / (2.0 * k), 700 / (2.0 * (700 - k))] for k in pos] + [list(COSTS), [1.0, 1.0]])  # 'balanced'
    x0, z0, u0 = _starts(np.random.default_rng(7), 57, 700, 12)
    o = dict(objevals=1, classes=classes, lossfunction=losses, x0=x0, z0=z0, u0=u0, classcost=cc)
    got = gpu.linearsvm_ovr(D, lab, Cv, dict(o, weights=w))
    steps = []
    for c in range(12):
        ref = R.run(D, ELL[:, c], Cv, R.cost_vector(ELL[:, c], w, cc[c]), losses[c],
                    dict(objevals=1, x0=x0[:, c], z0=z0[:, c], u0=u0[:, c]))
        steps.append(ref["steps"])
        _compare_class(got, c, ref)
    print("steps per class with shared weights:", steps)
    assert len(set(steps)) > 1  # they freeze at different times
    # 'balanced' as a string is the same K x 2 array for the first ten columns
    bal = gpu.linearsvm_ovr(D, lab, Cv, dict(o, classes=classes[:10], lossfunction=losses[:10], x0=x0[:, :10], z0=z0[:, :10],
                                             u0=u0[:, :10], classcost="balanced", weights=w))
    assert np.array_equal(bal["steps"], got["steps"][:10]) and np.array_equal(bal["xopt"], got["xopt"][:, :10])
    got = gpu.linearsvm_ovr(D, lab, Cv, o)
    ref = R.run(D, ELL[:, 10], Cv, R.cost_vector(ELL[:, 10], None, COSTS), "logistic",
                dict(objevals=1, x0=x0[:, 10], z0=z0[:, 10], u0=u0[:, 10]))
    _compare_class(got, 10, ref)
    ref = S.linearsvm(D, ELL[:, 11], Cv, dict(objevals=1, x0=x0[:, 11], z0=z0[:, 11], u0=u0[:, 11]))
    _compare_class(got, 11, ref)  # unit cost: unaffected by its neighbour's costs


def test_ovr_mixed_chunk_many_row_blocks(gpu, problems):
    """16385 x 8, columns 'sqhinge' with costs, hinge with unit cost, logistic with costs in one chunk, 20 forced
    iterations: the multi-block pass (ovr_pass_kernel<10, false, true, OvrCostArgs>)"""
    p = problems["16385x8"]
    D, ell, Cv = p["D"], p["ell"], p["C"]
    m, n = D.shape
    ELL = np.asfortranarray(np.stack([ell, ell, -ell], axis=1))
    losses = ["sqhinge", "hinge", "logistic"]
    cc = np.array([list(COSTS), [1.0, 1.0], [0.55, 5.07]])
    x0, z0, u0 = (np.asfortranarray(np.stack([p[k], p[k], p[k]], axis=1)) for k in ("x0", "z0", "u0"))
    L = gpu._lib
    obj = gpu.SvmOvr(D, ELL, Cv, losses)
    try:
        obj.set_cost(None, cc)
        summ = obj.run(maxiters=20, domaxiters=1, objevals=1, x0=x0, z0=z0, u0=u0)
        got = dict(steps=summ["steps"], objopt=summ["objopt"], xopt=obj.fetch(L.OVR_F_XOPT, n), zopt=obj.fetch(L.OVR_F_ZOPT, m),
                   uopt=obj.fetch(L.OVR_F_UOPT, m), pnorm=obj.fetch(L.OVR_F_PNORM, 20), perr=obj.fetch(L.OVR_F_PERR, 20),
                   Hnormsq=obj.fetch(L.OVR_F_HNORMSQ, 20), objevals=obj.fetch(L.OVR_F_OBJEVALS, 20))
    finally:
        obj.close()
    assert list(got["steps"]) == [20, 20, 20]
    o = dict(objevals=1, domaxiters=1, x0=p["x0"], z0=p["z0"], u0=p["u0"])
    for c in (0, 2):
        ref = R.run(D, ELL[:, c], Cv, R.cost_vector(ELL[:, c], None, cc[c]), losses[c], o, maxiters=20)
        _compare_class(got, c, ref, limit=20)
    ref = S.linearsvm(D, ell, Cv, o)
    for key in OVR_HIST:
        _err(f"{key}[1]", got[key][:20, 1], np.asarray(ref[key])[:20])
    for key, hist in (("xopt", "xvals"), ("zopt", "zvals"), ("uopt", "uvals")):
        _err(f"{key}[1]", got[key][:, 1], ref[hist][:, 19])


# ------------------------------------------------------------------------------------------------------ defaults
def test_defaults_launch_the_kernels_they_always_did(gpu, problems):
    """a default hinge run; the same engine after set_svm_cost(desc) and then set_svm_cost(NULL) repeats it bit for bit;
    explicit all-ones weights with costs (1, 1) -- the cost form of the kernel -- agree with it to 1e-12"""
    from admm_project_amd.solvers import _ENGINE_OBJ
    p = problems["700x57"]
    D, ell, m = p["D"], p["ell"], p["ell"].size
    gx, gz, _ = gpu.getproxops("LinearSVM", dict(D=D, ell=ell, C=p["C"], lossfunction="hinge"))
    eng = gx.problem.engine
    o = dict(A=D, At=D.T, B=-1, nB=m, c=0, m=m, maxiters=1000, stopcond="both", nodualerror=1, obj=_ENGINE_OBJ, objevals=1,
             x0=p["x0"], z0=p["z0"], u0=p["u0"])
    base = gpu.admm(gx, gz, dict(o))
    assert int(base["steps"]) == PLAIN_STEPS["700x57"]
    assert eng.svm_cost() == dict(classcost=(1.0, 1.0), has_weights=False)
    eng.set_svm_cost(p["w"], COSTS)
    assert eng.svm_cost() == dict(classcost=COSTS, has_weights=True)
    costly = gpu.admm(gx, gz, dict(o))
    assert int(costly["steps"]) != int(base["steps"])
    eng.set_svm_cost()
    assert eng.svm_cost() == dict(classcost=(1.0, 1.0), has_weights=False)
    again = gpu.admm(gx, gz, dict(o))
    assert int(again["steps"]) == int(base["steps"])
    for key in PLAIN + ("xopt", "zopt", "uopt"):
        assert np.array_equal(np.asarray(again[key]), np.asarray(base[key])), key
    eng.set_svm_cost(np.ones(m), (1.0, 1.0))
    assert eng.svm_cost()["has_weights"]
    ones = gpu.admm(gx, gz, dict(o))
    assert int(ones["steps"]) == int(base["steps"])
    for key in PLAIN + ("xopt", "zopt", "uopt"):
        _err(f"{key} (all-ones costs against the default)", ones[key], base[key], 1e-12)


# ------------------------------------------------------------------------------------------ C ABI and MEX gateway
def test_c_abi_refusals_change_nothing(gpu, ap, problems):
    L = ap._lib
    lib = L.load()
    p = problems["256x2"]
    m = p["ell"].size

    def in_force(eng):
        d, has = L.SvmCostDesc(), C.c_int32(-1)
        assert lib.admm_engine_get_svm_cost(eng._h, C.byref(d), C.byref(has)) == L.OK
        assert not d.weights
        return d.cost_pos, d.cost_neg, has.value

    eng = gpu.Engine(L.PROB_LINEARSVM, D=p["D"], ell=p["ell"], Cval=p["C"], loss=L.LOSS_SQHINGE)
    try:
        w = np.ones(m)
        good = L.SvmCostDesc(L.as_dp(w), 2.0, 0.5)
        assert lib.admm_engine_set_svm_cost(eng._h, C.byref(good)) == L.OK
        assert in_force(eng) == (2.0, 0.5, 1)
        neg = w.copy()
        neg[m // 2] = -1e-300
        for bad in (L.SvmCostDesc(L.as_dp(neg), 1.0, 1.0), L.SvmCostDesc(None, np.nan, 1.0),
                    L.SvmCostDesc(None, 1.0, np.inf), L.SvmCostDesc(None, -1.0, 1.0)):
            assert lib.admm_engine_set_svm_cost(eng._h, C.byref(bad)) == L.E_INVALID
            assert b"negative or not finite" in lib.admm_last_error()
            assert in_force(eng) == (2.0, 0.5, 1)  # the previous setting holds
        assert lib.admm_engine_set_svm_cost(eng._h, None) == L.OK
        assert in_force(eng) == (1.0, 1.0, 0)
    finally:
        eng.close()
    lad = gpu.Engine(L.PROB_LAD, D=p["D"], s=p["ell"])
    try:
        d = L.SvmCostDesc(None, 2.0, 0.5)
        assert lib.admm_engine_set_svm_cost(lad._h, C.byref(d)) == L.E_INVALID
        assert b"ADMM_PROB_LINEARSVM" in lib.admm_last_error()
        assert in_force(lad) == (1.0, 1.0, 0)
    finally:
        lad.close()


def test_c_abi_loss_values_and_ovr_costs(gpu, ap):
    """loss value 5 is accepted by admm_svm_ovr_create, 4 and 6 are refused; admm_svm_ovr_set_cost refuses a negative
    weight and a NaN cost"""
    L = ap._lib
    lib = L.load()
    rng = np.random.default_rng(0)
    D = np.asfortranarray(rng.random((64, 4)))
    E = np.asfortranarray(np.where(rng.random((64, 2)) < 0.5, 1.0, -1.0))
    for values, code in (((5, 4), L.E_INVALID), ((6, 0), L.E_INVALID), ((5, 5), L.OK), ((3, 5), L.OK)):
        loss = np.ascontiguousarray(values, dtype=np.int32)
        d = L.SvmOvrDesc()
        lib.admm_svm_ovr_desc_default(C.byref(d))
        d.K, d.m, d.n, d.D, d.ldD, d.C, d.ELL = 2, 64, 4, L.as_dp(D), 64, 0.5, L.as_dp(E)
        d.loss = loss.ctypes.data_as(C.POINTER(C.c_int32))
        h = C.c_void_p()
        rc = lib.admm_svm_ovr_create(C.byref(d), C.byref(h))
        assert rc == code, (values, rc)
        if code != L.OK:
            assert not h.value and b"bad loss for class" in lib.admm_last_error()
            continue
        w, cc = np.ones(64), np.ones((2, 2))
        assert lib.admm_svm_ovr_set_cost(h, L.as_dp(w), L.as_dp(cc)) == L.OK
        w[3], cc[1, 0] = -1.0, np.nan
        assert lib.admm_svm_ovr_set_cost(h, L.as_dp(w), None) == L.E_INVALID
        assert lib.admm_svm_ovr_set_cost(h, None, L.as_dp(cc)) == L.E_INVALID
        assert lib.admm_svm_ovr_set_cost(h, None, None) == L.OK
        lib.admm_svm_ovr_destroy(h)


def test_mex_gateway_costs(gpu, problems, tmp_path_factory):
    """as test_mex_gateway's LinearSVM case: args.weights, args.classcost and lossfunction = 'sqhinge' reach the binding
    unchanged"""
    from mexharness import Harness, build
    mex = Harness(build(tmp_path_factory.mktemp("mexcost")))
    p = problems["256x2"]
    D, ell, Cv = p["D"], p["ell"], p["C"]
    m = D.shape[0]
    args = dict(D=D, Dt=D.T, ell=ell, C=Cv, lossfunction="sqhinge", weights=p["w"], classcost=np.array(COSTS))
    options = dict(objevals=1, A=D, At=D.T, B=-1, nB=m, c=0, m=m, x0=p["x0"], z0=p["z0"], u0=p["u0"], maxiters=1000,
                   stopcond="both", nodualerror=1)
    got = mex.call("solve", "linearsvm", args, options, dict(objnative=1))
    ref = gpu.linearsvm(D, ell, Cv, dict(lossfunction="sqhinge", weights=p["w"], classcost=COSTS, objevals=1, x0=p["x0"],
                                         z0=p["z0"], u0=p["u0"]))
    assert int(got["steps"]) == int(ref["steps"])
    _err("xopt", got["xopt"], ref["xopt"], 1e-12)
    _err("objevals", got["objevals"], ref["objevals"], 1e-12)
