"""admm_svm_ovr where tests/test_gpu_svm_ovr.py does not reach: workgroups of the pass that take several 64-row blocks
(m > 16384), more than 16 partial rows in ovr_gsum_fin_kernel, the triangular-solve form of the x-update, a host D with
ldD > m, the default (zero) starts, the H-norm stop, and the refusals of fetch.

A. one iteration against a numpy.longdouble restatement of the plain-ADMM step (bound measured in the test: 50x the gap
   of the same step in float64 NumPy to the longdouble one, floor 1e-13),
B. many iterations on the multi-block path against oracle.solvers_ref.linearsvm at the 1e-7 of test_gpu_svm_ovr.py,
C. the triangular solves on a graded D (bound measured: 10x the gap between a chol(D'D) restatement and the oracle's
   pinv iterates, floor 1e-7),
D. ldD = m + 3 with NaN padding through the C ABI, bitwise against the compact run,
E. small behaviours of the object.

Figures measured on an MI355X are in EXPERIMENTS.md."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

from oracle import solvers_ref as S

pytestmark = pytest.mark.gpu

HIST = ("pnorm", "perr", "Hnormsq", "objevals")
LD = np.longdouble


def _relerr(got, ref):
    """vectors: max-norm error relative to the reference's max-norm; scalars: relative"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert not np.isnan(got.astype(np.float64)).any(), "NaN"
    return float(np.max(np.abs(got - ref)) / max(LD(1e-300), np.max(np.abs(ref))))


def _close(name, got, ref, tol):
    """the comparison of test_gpu_svm_ovr.py: scalar histories per entry, vectors in the max-norm"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert not np.isnan(got).any() and not np.isnan(ref).any(), f"{name}: NaN"
    if ref.ndim == 1 and not name.split("[")[0].endswith("opt"):
        scale = np.maximum(np.abs(ref), 1e-12 + 1e-3 * np.max(np.abs(ref)))
        err = float(np.max(np.abs(got - ref) / scale))
    else:
        err = float(np.max(np.abs(got - ref)) / max(1e-300, np.max(np.abs(ref))))
    print(f"{name}: relative error {err:.3e} (bound {tol:g})")
    assert err < tol, f"{name}: relative error {err:.3e} >= {tol:g}"
    return err


def _starts(rng, n, m, K):
    x0, z0, u0 = np.empty((n, K), order="F"), np.empty((m, K), order="F"), np.empty((m, K), order="F")
    for c in range(K):
        x0[:, c], z0[:, c], u0[:, c] = rng.random(n), rng.random(m), rng.random(m)
    return x0, z0, u0


def _fetch_table(L, n, m, S_, objevals=True):
    rows = (("xopt", L.OVR_F_XOPT, n), ("zopt", L.OVR_F_ZOPT, m), ("uopt", L.OVR_F_UOPT, m),
            ("pnorm", L.OVR_F_PNORM, S_), ("perr", L.OVR_F_PERR, S_), ("Hnormsq", L.OVR_F_HNORMSQ, S_))
    return rows + ((("objevals", L.OVR_F_OBJEVALS, S_),) if objevals else ())


def _fetch_all(gpu, obj, n, m, S_, objevals=True):
    return {key: obj.fetch(f, rows) for key, f, rows in _fetch_table(gpu._lib, n, m, S_, objevals)}


def _alternating(gpu, ell, starts):
    """K = chunk + 1 classes alternating between the labels and their negation; the last duplicates class 0"""
    K = gpu._lib.load().admm_svm_ovr_chunk() + 1
    src = [c % 2 for c in range(K)]
    src[-1] = 0
    ELL = np.asfortranarray(np.stack([ell if s == 0 else -ell for s in src], axis=1))
    return K, src, ELL, tuple(np.asfortranarray(v[:, src]) for v in starts)


# ------------------------------------------------------------------------------------- A. one iteration, exactly
def hinge_step(D, Dx, ell, Cc, rho, x, z0, u0, abstol, reltol):
    """one plain-ADMM step of the linear SVM after the x-update, in the precision of its arguments: the hinge z-prox
    (getProxOps.m:1094-1098), u, the sums of admm.m:612-658 with A = D, B = -1, c = 0, nodualerror, Hnormsq of
    admm.m:305-306 with w = [x; z; rho*u], and the objective of linearsvm.m:231-237"""
    T = Dx.dtype.type
    v = Dx + u0
    z = v + ell * np.maximum(np.minimum(1 - ell * v, T(Cc) / T(rho)), 0)
    u = u0 + (Dx - z)
    nrm = lambda a: np.sqrt(np.sum(a * a))
    m = T(Dx.size)
    return dict(xopt=x, zopt=z, uopt=u, pnorm=nrm(Dx - z),
                perr=np.sqrt(m) * T(abstol) + T(reltol) * max(nrm(Dx), nrm(z)),
                Hnormsq=T(rho) * np.sum((z - z0) ** 2) + T(rho) * np.sum((T(rho) * u - T(rho) * u0) ** 2),
                objevals=T(0.5) * np.sum(x * x) + T(Cc) * np.sum(np.maximum(1 - ell * Dx, 0)))


def one_step_refs(D, ell, Cc, z0, u0, rho=1.0, abstol=1e-5, reltol=1e-3):
    """(longdouble step, float64 step).  The longdouble x solves D'D x = D'(z0 - u0): a float64 Cholesky solve refined
    with longdouble residuals D'((z0 - u0) - D x) until the correction is below 1e-17 of x, which is a longdouble solve
    for the cond(D'D) < 1e3 of these matrices (each pass gains a factor cond * 2^-53)"""
    Dl, t = D.astype(LD), z0.astype(LD) - u0.astype(LD)
    G = D.T @ D
    cf = scipy.linalg.cho_factor(G)
    x = scipy.linalg.cho_solve(cf, D.T @ (z0 - u0)).astype(LD)
    for _ in range(6):
        dx = scipy.linalg.cho_solve(cf, (Dl.T @ (t - Dl @ x)).astype(np.float64)).astype(LD)
        x = x + dx
        if np.max(np.abs(dx)) <= LD(1e-17) * np.max(np.abs(x)):
            break
    else:
        raise AssertionError("the refinement of the longdouble solve did not settle")
    ref = hinge_step(Dl, Dl @ x, ell.astype(LD), Cc, rho, x, z0.astype(LD), u0.astype(LD), abstol, reltol)
    x64 = np.linalg.solve(G, D.T @ (z0 - u0))
    f64 = hinge_step(D, D @ x64, ell, Cc, rho, x64, z0, u0, abstol, reltol)
    return ref, f64


ONE_STEP_SHAPES = [(2048, 8), (2049, 8), (4096, 57), (4097, 57), (16384, 57), (16385, 57), (33000, 8), (16385, 447)]
# (the last entry: rho = 1.75, where rho, rho^3 and C / rho of the restatement differ from their values at rho = 1)
ONE_STEP_CASES = [(s, 1.0) for s in ONE_STEP_SHAPES] + [((16385, 57), 1.75)]
FIELDS = ("xopt", "zopt", "uopt") + HIST


@pytest.mark.parametrize("shape,rho", ONE_STEP_CASES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"rho{v}")
def test_one_iteration_against_longdouble(gpu, ap, shape, rho):
    """nwg = 32 | 33 (last block one row) | 64 | 65 (second trip of the gsum loop: one live row) | 256 workgroups, one
    block each | workgroup 0 takes a second block of one row | 516 blocks, ragged end | multi-block with the last
    column slot clamped.  Every field of every class is held to max(50 * gap, 1e-13), gap = the largest error over the
    fields of the float64 NumPy step against the longdouble one at this shape; 50x covers the different summation
    order of up to 256 partials."""
    m, n = shape
    p = ap.synth.mnist_like_problem(seed=1, m=m, n=n)
    D, ell, Cc = p["D"], p["ell"], p["C"]
    x0, z0, u0 = _starts(np.random.default_rng(11), n, m, 2)
    refs = [one_step_refs(D, e, Cc, z0[:, s], u0[:, s], rho=rho) for s, e in enumerate((ell, -ell))]
    K, src, ELL, (X0, Z0, U0) = _alternating(gpu, ell, (x0, z0, u0))
    obj = gpu.SvmOvr(D, ELL, Cc, ["hinge"] * K)
    try:
        summ = obj.run(rho=rho, maxiters=1, domaxiters=1, objevals=1, x0=X0, z0=Z0, u0=U0)
        got = _fetch_all(gpu, obj, n, m, 1)
    finally:
        obj.close()
    assert list(summ["steps"]) == [1] * K
    gaps = {key: max(_relerr(refs[s][1][key], refs[s][0][key]) for s in (0, 1)) for key in FIELDS}
    gap = max(gaps.values())
    bound = max(50.0 * gap, 1e-13)
    errs = {key: max(_relerr(got[key][:, c] if key.endswith("opt") else got[key][0, c], refs[src[c]][0][key])
                     for c in range(K)) for key in FIELDS}
    for key in FIELDS:
        print(f"A {m}x{n} rho {rho} {key}: float64 gap {gaps[key]:.3e}, kernel error {errs[key]:.3e}")
    print(f"A {m}x{n} rho {rho}: float64 gap {gap:.3e}, kernel error {max(errs.values()):.3e}, bound {bound:.3e}")
    for key in FIELDS:
        assert errs[key] <= bound, f"{key}: {errs[key]:.3e} > {bound:.3e}"
    for c in range(K):
        assert summ["objopt"][c] == got["objevals"][0, c]
    for key in FIELDS:
        assert np.array_equal(got[key][:, K - 1], got[key][:, 0]), key  # the duplicate in the second chunk: bitwise


# ------------------------------------------------------------------- B. many iterations on the multi-block path
def _compare_class(got, c, ref, tol, limit=None):
    k = int(got["steps"][c]) if limit is None else limit
    for key in HIST:
        _close(f"{key}[{c}]", got[key][:k, c], np.asarray(ref[key])[:k], tol)
    if limit is None:
        for key in HIST:
            assert np.isnan(got[key][k:, c]).all(), (key, c)  # NaN past the class's last step
        for key in ("xopt", "zopt", "uopt"):
            _close(f"{key}[{c}]", got[key][:, c], ref[key], tol)
        _close(f"objopt[{c}]", [got["objopt"][c]], [ref["objopt"]], tol)
    else:
        for key, hist in (("xopt", "xvals"), ("zopt", "zvals"), ("uopt", "uvals")):
            _close(f"{key}[{c}]", got[key][:, c], ref[hist][:, k - 1], tol)
        _close(f"objopt[{c}]", [got["objopt"][c]], [ref["objevals"][k - 1]], tol)


FORCED = 25


@pytest.fixture(scope="module")
def forced_refs(ap):
    """the oracle's runs for the two label vectors per shape, computed once.  The oracle runs to ITS stop (more than 25
    steps at these shapes, asserted): the first 25 iterates of a run do not depend on where it stops, and 1000 forced
    steps would hold 4 m x 1000 doubles of vector histories per run (1 GB at m = 33000)"""
    out = {}
    for m, n in ((16385, 57), (33000, 8)):
        p = ap.synth.mnist_like_problem(seed=1, m=m, n=n)
        x0, z0, u0 = _starts(np.random.default_rng(11), n, m, 2)
        refs = [S.linearsvm(p["D"], e, p["C"], dict(objevals=1, x0=x0[:, c], z0=z0[:, c], u0=u0[:, c]))
                for c, e in enumerate((p["ell"], -p["ell"]))]
        out[(m, n)] = dict(D=p["D"], ell=p["ell"], C=p["C"], starts=(x0, z0, u0), refs=refs)
    return out


@pytest.mark.parametrize("shape", [(16385, 57), (33000, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_forced_iterations_multi_block(gpu, forced_refs, shape):
    e = forced_refs[shape]
    m, n = shape
    K, src, ELL, (X0, Z0, U0) = _alternating(gpu, e["ell"], e["starts"])
    obj = gpu.SvmOvr(e["D"], ELL, e["C"], ["hinge"] * K)
    try:
        summ = obj.run(maxiters=FORCED, domaxiters=1, objevals=1, x0=X0, z0=Z0, u0=U0)
        got = dict(_fetch_all(gpu, obj, n, m, FORCED), steps=summ["steps"], objopt=summ["objopt"])
    finally:
        obj.close()
    assert list(got["steps"]) == [FORCED] * K and not summ["stopped_early"].any()
    for c in range(K):
        ref = e["refs"][src[c]]
        assert ref["steps"] >= FORCED, ref["steps"]
        _compare_class(got, c, ref, 1e-7, limit=FORCED)
    for key in FIELDS:
        assert np.array_equal(got[key][:, K - 1], got[key][:, 0]), key


def test_classes_freeze_on_the_multi_block_path(gpu, ap):
    """16385 x 8, eleven classes with their own labels and random starts, run to convergence: the classes stop at
    different iterations (asserted on the oracle, so a loop that never freezes cannot pass), and a frozen class must
    keep its columns while workgroup 0 goes on taking its second block for the others"""
    m, n, K = 16385, 8, 11
    p = ap.synth.mnist_like_problem(seed=1, m=m, n=n)
    rng = np.random.default_rng(5)
    labels = rng.integers(0, K, size=m).astype(np.float64)
    x0, z0, u0 = _starts(rng, n, m, K)
    refs = [S.linearsvm(p["D"], np.where(labels == c, 1.0, -1.0), p["C"],
                        dict(objevals=1, x0=x0[:, c], z0=z0[:, c], u0=u0[:, c])) for c in range(K)]
    steps = [r["steps"] for r in refs]
    print("oracle steps:", steps)
    assert len(set(steps)) > 1
    got = gpu.linearsvm_ovr(p["D"], labels, p["C"], dict(objevals=1, x0=x0, z0=z0, u0=u0))
    assert np.array_equal(got["classes"], np.arange(float(K)))
    assert list(got["steps"]) == steps
    assert got["pnorm"].shape == (max(steps), K)
    for c in range(K):
        _compare_class(got, c, refs[c], 1e-7)


# ------------------------------------------------------------------------ C. the triangular-solve form of the x-update
def restated_run(D, ell, Cc, loss, x0, z0, u0, steps, rho=1.0):
    """`steps` iterations of the linear SVM with x = (D'D)^-1 D'(z - u) through scipy's Cholesky factor of D'D
    (what the device's triangular solves compute) instead of the oracle's pinv(D)"""
    cf = scipy.linalg.cho_factor(D.T @ D)
    z, u = z0.copy(), u0.copy()
    h = {k: [] for k in ("xvals", "zvals", "uvals", "pnorm")}
    for _ in range(steps):
        x = scipy.linalg.cho_solve(cf, D.T @ (z - u))
        Dx = D @ x
        v = ell * (Dx + u)
        if loss == "hinge":
            z = Dx + u + ell * np.maximum(np.minimum(1 - v, Cc / rho), 0.0)
        else:
            z = ell * np.where((v >= 1) | (v < 1 - np.sqrt(2.0 * Cc / rho)), v, 1.0)
        u = u + (Dx - z)
        for k, a in (("xvals", x), ("zvals", z), ("uvals", u)):
            h[k].append(a.copy())
        h["pnorm"].append(np.sqrt(np.sum((Dx - z) ** 2)))
    return {k: np.stack(a, axis=-1) for k, a in h.items()}


def guarded_prefix(D, ell, Cc, ref, u0, cap=40):
    """the number of leading iterations of a 0-1 run over which no component sits within 1e-6 of a decision boundary
    of minz01 (getProxOps.m:1175), as test_01_and_mixed_losses_margin_guarded takes it"""
    k, u = 0, u0
    for i in range(min(ref["steps"], cap)):
        sarg = ell * (D @ ref["xvals"][:, i] + u)
        if min(np.min(np.abs(sarg - 1.0)), np.min(np.abs(sarg - (1 - np.sqrt(2.0 * Cc))))) < 1e-6:
            break
        u = ref["uvals"][:, i]
        k = i + 1
    return k


TRSV_KAPPA, TRSV_SEED = 1e5, 165
TRSV_LOSSES = ["hinge", "hinge", "01"]


def trsv_problem(ap):
    m, n, K = 700, 57, 3
    D = ap.synth.graded_matrix(TRSV_SEED, m, n, TRSV_KAPPA)
    rng = np.random.default_rng(TRSV_SEED + 100)
    labels = rng.integers(0, K, size=m).astype(np.float64)
    x0, z0, u0 = _starts(rng, n, m, K)
    return dict(D=D, C=0.5, labels=labels, x0=x0, z0=z0, u0=u0,
                ell=[np.where(labels == c, 1.0, -1.0) for c in range(K)])


def trsv_refs(d):
    """per class: the oracle's run, the number of steps compared (all for hinge, the guarded prefix for 0-1), and the
    gap of the Cholesky restatement to the oracle's pinv iterates over those steps"""
    out = []
    for c, loss in enumerate(TRSV_LOSSES):
        ref = S.linearsvm(d["D"], d["ell"][c], d["C"], dict(objevals=1, lossfunction=loss, x0=d["x0"][:, c],
                                                          z0=d["z0"][:, c], u0=d["u0"][:, c]))
        k = ref["steps"] if loss == "hinge" else guarded_prefix(d["D"], d["ell"][c], d["C"], ref, d["u0"][:, c])
        re = restated_run(d["D"], d["ell"][c], d["C"], loss, d["x0"][:, c], d["z0"][:, c], d["u0"][:, c], k)
        gap = 0.0
        for key in ("xvals", "zvals", "uvals"):
            a, b = re[key], ref[key][:, :k]
            gap = max(gap, float(np.max(np.max(np.abs(a - b), axis=0) / np.max(np.abs(b), axis=0))))
        gap = max(gap, float(np.max(np.abs(re["pnorm"] - ref["pnorm"][:k]) / ref["pnorm"][:k])))
        out.append(dict(ref=ref, k=k, gap=gap))
    return out


def test_triangular_solve_form(gpu, ap):
    """a graded D on which create's accuracy probe keeps the triangular solves: the o->M == nullptr form,
    launch_trsv_pair per class and ovr_xcopy_kernel, run to convergence so that classes freeze at different steps
    while the copy runs.  Two hinge classes in full, one 0-1 class over its margin-guarded prefix.

    On graded matrices both forms of the x-update lose the same digits and create keeps the explicit inverse nearly
    always: of seeds 0-399 at 700 x 57 none reaches the triangular solves at kappa 1e3 (0-39) or 1e4, and two do at
    1e5: 165 (probe errors inverse / trsv 8.74e-8 / 3.77e-8, kept while inverse <= 2 * trsv) and 289 (2.95e-7 /
    1.39e-7).  Hence kappa = 1e5, seed 165.  If a change to the probe or the factorization makes the first assertion
    fail, pick the seed again: create an Engine(PROB_LINEARSVM) on graded_matrix(seed, 700, 57, kappa) for the seeds
    and the three kappas, read info()["xsolve_used"], and take the smallest kappa and a seed whose probe errors are
    well apart from the threshold (EXPERIMENTS.md has the last scan).
    The bound at this kappa: the Cholesky restatement is 1.5e-5 from the oracle's pinv iterates over the 116 / 122
    steps, so 1.5e-4; no stop decision of the oracle's hinge runs is nearer than 4.5e-3 to its threshold.  What the
    bound still sees: a class that took one more x-update after its stop (ovr_xcopy_kernel not skipping it) would
    have its x moved by 2.4e-3 (class 0) and 9.5e-4 (class 1), 16 and 6 times the bound."""
    d = trsv_problem(ap)
    m, n = d["D"].shape
    eng = gpu.engine.Engine(gpu._lib.PROB_LINEARSVM, D=d["D"], ell=d["ell"][0], Cval=d["C"])
    try:
        info = eng.info()
    finally:
        eng.close()
    print("probe:", {k: info[k] for k in ("xsolve_used", "probe_err_inverse", "probe_err_trsv", "probe_diff",
                                          "cond_estimate")})
    assert info["xsolve_used"] == "trsv", info  # the same create the object runs: it is on the path under test
    refs = trsv_refs(d)
    gap = max(r["gap"] for r in refs)
    tol = max(10.0 * gap, 1e-7)
    print(f"C: Cholesky restatement against the oracle's pinv iterates: gap {gap:.3e}, bound {tol:.3e}")
    hinge = [c for c, v in enumerate(TRSV_LOSSES) if v == "hinge"]
    for c in hinge:  # no stop decision of a compared class within the bound of its threshold (chosen by TRSV_SEED)
        r = refs[c]["ref"]
        assert np.min(np.abs(r["pnorm"] - r["perr"]) / r["perr"]) > tol, c
        assert np.min(np.abs(r["Hnormsq"][2:] - 1e-6) / 1e-6) > tol, c
    assert len({refs[c]["ref"]["steps"] for c in hinge}) > 1
    got = gpu.linearsvm_ovr(d["D"], d["labels"], d["C"], dict(objevals=1, lossfunction=TRSV_LOSSES, x0=d["x0"],
                                                             z0=d["z0"], u0=d["u0"]))
    print("steps:", list(got["steps"]), "oracle:", [r["ref"]["steps"] for r in refs])
    for c in hinge:
        assert got["steps"][c] == refs[c]["ref"]["steps"]
        _compare_class(got, c, refs[c]["ref"], tol)
    c = TRSV_LOSSES.index("01")
    k = refs[c]["k"]
    assert k >= 10, k
    assert got["steps"][c] >= k
    for key in ("pnorm", "perr", "Hnormsq", "objevals"):
        _close(f"{key}[{c}]", got[key][:k, c], np.asarray(refs[c]["ref"][key])[:k], tol)


# ---------------------------------------------------------------------------------- D. ldD > m through the C ABI
def _abi_run(L, lib, Dbuf, ldD, m, n, ELL, Cc, x0, z0, u0, iters):
    d = L.SvmOvrDesc()
    lib.admm_svm_ovr_desc_default(C.byref(d))
    K = ELL.shape[1]
    d.K, d.m, d.n, d.D, d.ldD, d.ELL, d.C = K, m, n, L.as_dp(Dbuf), ldD, L.as_dp(ELL), Cc
    h = C.c_void_p()
    L.check(lib.admm_svm_ovr_create(C.byref(d), C.byref(h)))
    try:
        o = L.SvmOvrOptions()
        lib.admm_svm_ovr_options_default(C.byref(o))
        o.maxiters, o.domaxiters, o.objevals = iters, 1, 1
        o.x0, o.z0, o.u0 = L.as_dp(x0), L.as_dp(z0), L.as_dp(u0)
        summ = (L.SvmOvrSummary * K)()
        L.check(lib.admm_svm_ovr_run(h, C.byref(o), summ, None))
        out = dict(steps=np.array([s.steps for s in summ]), objopt=np.array([s.objopt for s in summ]))
        for key, f, rows in _fetch_table(L, n, m, iters):
            buf = np.empty((rows, K), order="F")
            w = C.c_size_t(0)
            L.check(lib.admm_svm_ovr_fetch(h, f, L.as_dp(buf), buf.size, C.byref(w)))
            assert w.value == buf.size
            out[key] = buf
        return out
    finally:
        lib.admm_svm_ovr_destroy(h)


@pytest.mark.parametrize("shape", [(37, 5), (16385, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_leading_dimension_through_the_c_abi(gpu, shape):
    """D in a buffer of ldD = m + 3 rows per column, the three padding rows NaN: every fetched field equals the run on
    the compact D bitwise, and no NaN comes back"""
    m, n = shape
    L, lib = gpu._lib, gpu._lib.load()
    p = gpu.synth.mnist_like_problem(seed=1, m=m, n=n)
    ELL = np.asfortranarray(np.stack([p["ell"], -p["ell"]], axis=1))
    x0, z0, u0 = _starts(np.random.default_rng(11), n, m, 2)
    padded = np.full((m + 3, n), np.nan, order="F")
    padded[:m, :] = p["D"]
    a = _abi_run(L, lib, np.asfortranarray(p["D"]), m, m, n, ELL, p["C"], x0, z0, u0, 10)
    b = _abi_run(L, lib, padded, m + 3, m, n, ELL, p["C"], x0, z0, u0, 10)
    assert list(a["steps"]) == [10, 10] and list(b["steps"]) == [10, 10]
    for key in a:
        assert not np.isnan(b[key]).any(), key
        assert np.array_equal(a[key], b[key]), key


# ------------------------------------------------------------------------------- E. small behaviours of the object
@pytest.fixture(scope="module")
def small(ap):
    p, q = (ap.synth.mnist_like_problem(seed=1, m=700, n=57, digit=d) for d in (0, 1))  # same D, digits 0 and 1
    assert np.array_equal(p["D"], q["D"])
    ELL = np.asfortranarray(np.stack([p["ell"], q["ell"]], axis=1))
    return dict(D=p["D"], C=p["C"], ELL=ELL)


def test_default_starts(gpu, small):
    """no x0 / z0 / u0: the object starts from zeros, the defaults of admm.m:252-259 (oracle/admm_ref.py).  The
    oracle's linearsvm cannot be left to its own defaults here: unwrappedadmm.m:87-89 draws random starts whenever
    none are given (solvers_ref.unwrappedadmm does the same), so it is handed the zeros explicitly"""
    m, n = small["D"].shape
    obj = gpu.SvmOvr(small["D"], small["ELL"], small["C"], ["hinge", "hinge"])
    try:
        summ = obj.run(objevals=1)
        S_ = int(summ["steps"].max())
        got = dict(_fetch_all(gpu, obj, n, m, S_), steps=summ["steps"], objopt=summ["objopt"])
    finally:
        obj.close()
    for c in range(2):
        ref = S.linearsvm(small["D"], small["ELL"][:, c], small["C"],
                          dict(objevals=1, x0=np.zeros(n), z0=np.zeros(m), u0=np.zeros(m)))
        assert got["steps"][c] == ref["steps"]
        _compare_class(got, c, ref, 1e-7)


HNORM_OPTS = dict(Hnormtol=1e-2, abstol=1e-12, reltol=1e-12)


def test_hnorm_stop(gpu, small):
    """a large Hnormtol and tiny abstol / reltol: the branch i > 2 && Hnormsq <= Hnormtol is what stops the classes"""
    m, n = small["D"].shape
    x0, z0, u0 = _starts(np.random.default_rng(7), n, m, 2)
    obj = gpu.SvmOvr(small["D"], small["ELL"], small["C"], ["hinge", "hinge"])
    try:
        summ = obj.run(objevals=1, x0=x0, z0=z0, u0=u0, **HNORM_OPTS)
        S_ = int(summ["steps"].max())
        got = dict(_fetch_all(gpu, obj, n, m, S_), steps=summ["steps"], objopt=summ["objopt"])
    finally:
        obj.close()
    for c in range(2):
        ref = S.linearsvm(small["D"], small["ELL"][:, c], small["C"],
                          dict(objevals=1, x0=x0[:, c], z0=z0[:, c], u0=u0[:, c], **HNORM_OPTS))
        k = ref["steps"]
        assert 3 <= k < 1000
        assert ref["pnorm"][-1] >= ref["perr"][-1] and ref["Hnormsq"][-1] <= HNORM_OPTS["Hnormtol"]  # the H-norm stop
        assert got["steps"][c] == k and summ["stopped_early"][c] == 1
        _compare_class(got, c, ref, 1e-7)


def test_maxiters_between_polls(gpu, small):
    """maxiters = 11 with check_every = 4: the last poll comes at an iteration that is no multiple of check_every,
    with both classes still running"""
    m, n = small["D"].shape
    x0, z0, u0 = _starts(np.random.default_rng(7), n, m, 2)
    obj = gpu.SvmOvr(small["D"], small["ELL"], small["C"], ["hinge", "hinge"])
    try:
        summ = obj.run(maxiters=11, check_every=4, x0=x0, z0=z0, u0=u0)
        pn = obj.fetch(gpu._lib.OVR_F_PNORM, 11)
        pe = obj.fetch(gpu._lib.OVR_F_PERR, 11)
    finally:
        obj.close()
    assert (pn >= pe).all()  # neither class met the stop test
    assert list(summ["steps"]) == [11, 11] and list(summ["stopped_early"]) == [0, 0]


def test_fetch_refusals(gpu, small):
    L, lib = gpu._lib, gpu._lib.load()
    m, n = small["D"].shape
    obj = gpu.SvmOvr(small["D"], small["ELL"], small["C"], ["hinge", "hinge"])
    buf = np.empty(2 * m)
    w = C.c_size_t(0)

    def refused(field, cap, code):
        rc = lib.admm_svm_ovr_fetch(obj._h, field, L.as_dp(buf), cap, C.byref(w))
        assert rc == code, (rc, code)
        msg = lib.admm_last_error()
        assert msg and len(msg) > 0

    try:
        refused(L.OVR_F_XOPT, buf.size, L.E_INVALID)  # before the first run
        summ = obj.run(maxiters=5, domaxiters=1, objevals=0)
        assert list(summ["steps"]) == [5, 5]
        refused(L.OVR_F_XOPT, 2 * n - 1, L.E_CAPACITY)
        refused(L.OVR_F_ZOPT, 2 * m - 1, L.E_CAPACITY)
        refused(L.OVR_F_PNORM, 2 * 5 - 1, L.E_CAPACITY)
        refused(L.OVR_F_OBJEVALS, buf.size, L.E_INVALID)  # objevals = 0
        refused(0, buf.size, L.E_INVALID)
        refused(99, buf.size, L.E_INVALID)
        assert obj.fetch(L.OVR_F_XOPT, n).shape == (n, 2)  # the object still answers
    finally:
        obj.close()
