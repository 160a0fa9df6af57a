"""linearsvm_ovr / admm_svm_ovr: K one-vs-rest linear SVMs in one run over D, per class against the CPU oracle
(oracle.solvers_ref.linearsvm with that class's ell, loss, start columns and the same options).

Tolerances are the single-class path's own: 1e-7 for a full-rank D (test_svm_hinge: pinv(D)(z-u) against the
chol(D'D) solve, kappa(D)^2 * eps apart), 1e-6 for a rank-deficient D (test_svm_rank_deficient_matches_pinv)."""
import ctypes as C

import numpy as np
import pytest

from oracle import solvers_ref as S

pytestmark = pytest.mark.gpu

HIST = ("pnorm", "perr", "Hnormsq", "objevals")


def _close(name, got, ref, tol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert not np.isnan(got).any() and not np.isnan(ref).any(), f"{name}: NaN"
    if ref.ndim == 1 and not name.endswith("opt"):
        scale = np.maximum(np.abs(ref), 1e-12 + 1e-3 * np.max(np.abs(ref)))  # scalar histories: per entry
        err = float(np.max(np.abs(got - ref) / scale))
    else:
        err = float(np.max(np.abs(got - ref)) / max(1e-300, np.max(np.abs(ref))))
    print(f"{name}: relative error {err:.3e} (bound {tol:g})")
    assert err < tol, f"{name}: relative error {err:.3e} >= {tol:g}"


def _starts(rng, n, m, K):
    """x0, z0, u0 columns drawn per class in the order x0, z0, u0"""
    x0, z0, u0 = np.empty((n, K), order="F"), np.empty((m, K), order="F"), np.empty((m, K), order="F")
    for c in range(K):
        x0[:, c], z0[:, c], u0[:, c] = rng.random(n), rng.random(m), rng.random(m)
    return x0, z0, u0


def _compare_class(got, c, ref, tol, keys=HIST, limit=None):
    """column c of an OvR result against one oracle run, over the class's own steps (or the first `limit`)"""
    k = int(got["steps"][c]) if limit is None else limit
    for key in keys:
        if key in ref:
            _close(f"{key}[{c}]", got[key][:k, c], np.asarray(ref[key])[:k], tol)
    if limit is None:
        assert np.isnan(got["pnorm"][k:, c]).all()  # NaN past the class's last step
        for key in ("xopt", "zopt", "uopt"):
            _close(f"{key}[{c}]", got[key][:, c], ref[key], tol)
        if "objopt" in ref:
            _close(f"objopt[{c}]", [got["objopt"][c]], [ref["objopt"]], tol)


@pytest.fixture(scope="module")
def digits(ap):
    """700 x 57 pixels with the reference's MNIST labels, classes 0-9, and the oracle's ten hinge runs"""
    labels = ap.synth.reference_mnist_labels("train")
    p = ap.synth.mnist_like_problem(seed=1, m=700, n=57, labels=labels)
    lab = np.asarray(labels[:700], dtype=np.float64)
    x0, z0, u0 = _starts(np.random.default_rng(7), 57, 700, 10)
    d = dict(D=p["D"], C=p["C"], labels=lab, x0=x0, z0=z0, u0=u0, hinge=[], ell=[])
    for c in range(10):
        ell = np.where(lab == c, 1.0, -1.0)
        d["ell"].append(ell)
        d["hinge"].append(S.linearsvm(p["D"], ell, p["C"], dict(objevals=1, x0=x0[:, c], z0=z0[:, c], u0=u0[:, c])))
    return d


def test_hinge_classes_stop_at_different_times(gpu, digits):
    """the test of freezing: a class that kept updating after its stop fails it"""
    d = digits
    assert [r["steps"] for r in d["hinge"]] == [73, 56, 69, 67, 62, 68, 65, 67, 66, 71]
    got = gpu.linearsvm_ovr(d["D"], d["labels"], d["C"], dict(objevals=1, classes=np.arange(10.0), x0=d["x0"],
                                                             z0=d["z0"], u0=d["u0"]))
    assert np.array_equal(got["classes"], np.arange(10.0))
    assert list(got["steps"]) == [r["steps"] for r in d["hinge"]]
    assert got["pnorm"].shape == (73, 10)
    for c in range(10):
        _compare_class(got, c, d["hinge"][c], 1e-7)


def test_01_and_mixed_losses_margin_guarded(gpu, digits):
    """twenty columns: every class with hinge and with 01.  The 0-1 prox is discontinuous (q24): its columns are
    compared over the first k iterations, where no component sits within 1e-6 of a decision boundary of minz01
    (getProxOps.m:1175), as test_svm_01_margin_guarded does; hinge columns in full"""
    d = digits
    D, Cc = d["D"], d["C"]
    classes = np.repeat(np.arange(10.0), 2)
    losses = ["hinge", "01"] * 10
    x0, z0, u0 = (np.asfortranarray(np.repeat(d[k], 2, axis=1)) for k in ("x0", "z0", "u0"))
    got = gpu.linearsvm_ovr(D, d["labels"], Cc, dict(objevals=1, classes=classes, lossfunction=losses, x0=x0, z0=z0,
                                                    u0=u0))
    for c in range(10):
        _compare_class(got, 2 * c, d["hinge"][c], 1e-7)  # unaffected by the 0-1 neighbours
        ell = d["ell"][c]
        ref = S.linearsvm(D, ell, Cc, dict(objevals=1, lossfunction="01", x0=d["x0"][:, c], z0=d["z0"][:, c],
                                           u0=d["u0"][:, c]))
        k, u = 0, d["u0"][:, c]
        for i in range(min(ref["steps"], 40)):
            sarg = ell * (D @ ref["xvals"][:, i] + u)
            margin = min(np.min(np.abs(sarg - 1.0)), np.min(np.abs(sarg - (1 - np.sqrt(2.0 * Cc)))))
            if margin < 1e-6:
                break
            u = ref["uvals"][:, i]
            k = i + 1
        assert k >= 10, (c, k)
        assert got["steps"][2 * c + 1] >= k
        _compare_class(got, 2 * c + 1, ref, 1e-7, keys=("pnorm", "perr", "objevals"), limit=k)


def _edge_problem(ap, m, n):
    if (m, n) == (256, 2):
        p = ap.synth.svm_problem(0)
        return p["D"], p["ell"], p["C"]
    p = ap.synth.mnist_like_problem(seed=1, m=m, n=n)
    return p["D"], p["ell"], p["C"]


@pytest.fixture(scope="module")
def edge_refs(ap):
    """the oracle's forced 1000 iterations per edge shape (class 0, class 1 = the flipped labels), computed once"""
    out = {}
    for m, n in ((37, 5), (129, 8), (256, 2), (1000, 448), (1000, 447)):
        D, ell, Cc = _edge_problem(ap, m, n)
        x0, z0, u0 = _starts(np.random.default_rng(11), n, m, 2)
        refs = [S.linearsvm(D, e, Cc, dict(objevals=1, domaxiters=1, x0=x0[:, c], z0=z0[:, c], u0=u0[:, c]))
                for c, e in enumerate((ell, -ell))]
        out[(m, n)] = dict(D=D, ell=ell, C=Cc, x0=x0, z0=z0, u0=u0, refs=refs)
    return out


@pytest.mark.parametrize("kind", ["one", "chunk", "chunk+1"])
@pytest.mark.parametrize("shape", [(37, 5), (129, 8), (256, 2), (1000, 448), (1000, 447)])
def test_shapes_at_the_kernels_edges(gpu, edge_refs, shape, kind):
    """fewer rows than a block; one row into a third block with n = the wave count; svm_problem(0); n at the limit and
    one below.  K = 1, K = chunk, K = chunk + 1 with classes alternating between the labels and their negation; for
    chunk + 1 the last class duplicates class 0 and must equal it bitwise: a class gets the same numbers whichever
    chunk and slot it lands in"""
    e = edge_refs[shape]
    m, n = shape
    kc = gpu._lib.load().admm_svm_ovr_chunk()
    K = {"one": 1, "chunk": kc, "chunk+1": kc + 1}[kind]
    src = [c % 2 for c in range(K)]
    if kind == "chunk+1":
        src[-1] = 0
    ELL = np.asfortranarray(np.stack([e["ell"] if s == 0 else -e["ell"] for s in src], axis=1))
    x0, z0, u0 = (np.asfortranarray(e[k][:, src]) for k in ("x0", "z0", "u0"))
    obj = gpu.SvmOvr(e["D"], ELL, e["C"], ["hinge"] * K)
    try:
        summ = obj.run(maxiters=25, domaxiters=1, objevals=1, x0=x0, z0=z0, u0=u0)
        got = dict(steps=summ["steps"], xopt=obj.fetch(gpu._lib.OVR_F_XOPT, n), zopt=obj.fetch(gpu._lib.OVR_F_ZOPT, m),
                   uopt=obj.fetch(gpu._lib.OVR_F_UOPT, m), pnorm=obj.fetch(gpu._lib.OVR_F_PNORM, 25),
                   perr=obj.fetch(gpu._lib.OVR_F_PERR, 25), Hnormsq=obj.fetch(gpu._lib.OVR_F_HNORMSQ, 25),
                   objevals=obj.fetch(gpu._lib.OVR_F_OBJEVALS, 25), objopt=summ["objopt"])
    finally:
        obj.close()
    assert list(got["steps"]) == [25] * K and not summ["stopped_early"].any()
    for c in sorted(set([0, 1, K - 2, K - 1]) & set(range(K))):
        ref = e["refs"][src[c]]
        assert ref["steps"] == 1000
        _compare_class(got, c, ref, 1e-7, limit=25)
        for key, hist in (("xopt", "xvals"), ("zopt", "zvals"), ("uopt", "uvals")):
            _close(f"{key}[{c}]", got[key][:, c], ref[hist][:, 24], 1e-7)
        _close(f"objopt[{c}]", [got["objopt"][c]], [ref["objevals"][24]], 1e-7)
    if kind == "chunk+1":
        for key in ("xopt", "zopt", "uopt") + HIST:
            assert np.array_equal(got[key][:, K - 1], got[key][:, 0]), key
        assert got["objopt"][K - 1] == got["objopt"][0]


def test_rank_deficient(gpu):
    p = gpu.synth.rank_deficient_pixels(seed=1, m=600, n=100, digit=3)
    assert np.linalg.matrix_rank(p["D"]) == p["rank"] < 100
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 3, size=600).astype(np.float64)
    x0, z0, u0 = _starts(rng, 100, 600, 3)
    got = gpu.linearsvm_ovr(p["D"], labels, p["C"], dict(objevals=1, x0=x0, z0=z0, u0=u0))
    assert list(got["classes"]) == [0.0, 1.0, 2.0]
    for c in range(3):
        ell = np.where(labels == c, 1.0, -1.0)
        ref = S.linearsvm(p["D"], ell, p["C"], dict(objevals=1, x0=x0[:, c], z0=z0[:, c], u0=u0[:, c]))
        assert got["steps"][c] == ref["steps"]
        _compare_class(got, c, ref, 1e-6)


def test_callers_pseudo_inverse(gpu, digits):
    """options.Dplus = numpy.linalg.pinv(D) is what the x-update is built from (linearsvm.m:185-186)"""
    d = digits
    o = dict(objevals=1, classes=[0.0, 1.0, 2.0], x0=d["x0"][:, :3], z0=d["z0"][:, :3], u0=d["u0"][:, :3])
    got = gpu.linearsvm_ovr(d["D"], d["labels"], d["C"], dict(o, Dplus=np.linalg.pinv(d["D"])))
    for c in range(3):
        assert got["steps"][c] == d["hinge"][c]["steps"]
        _compare_class(got, c, d["hinge"][c], 1e-7)


def _run_all(gpu, obj, n, m, **kw):
    summ = obj.run(**kw)
    L = gpu._lib
    S_ = int(summ["steps"].max())
    out = dict(steps=summ["steps"], objopt=summ["objopt"])
    for key, f, rows in (("xopt", L.OVR_F_XOPT, n), ("zopt", L.OVR_F_ZOPT, m), ("uopt", L.OVR_F_UOPT, m),
                         ("pnorm", L.OVR_F_PNORM, S_), ("perr", L.OVR_F_PERR, S_), ("Hnormsq", L.OVR_F_HNORMSQ, S_)):
        out[key] = obj.fetch(f, rows)
    if kw.get("objevals"):
        out["objevals"] = obj.fetch(L.OVR_F_OBJEVALS, S_)
    return out


def test_rerun_check_every_and_objevals(gpu, digits):
    d = digits
    ELL = np.asfortranarray(np.stack(d["ell"][:4], axis=1))
    kw = dict(x0=d["x0"][:, :4], z0=d["z0"][:, :4], u0=d["u0"][:, :4])
    a = gpu.SvmOvr(d["D"], ELL, d["C"], ["hinge", "01", "hinge", "hinge"])
    b = gpu.SvmOvr(d["D"], ELL, d["C"], ["hinge", "01", "hinge", "hinge"])
    try:
        first = _run_all(gpu, a, 57, 700, rho=1.0, objevals=1, **kw)
        second = _run_all(gpu, a, 57, 700, rho=2.0, objevals=1, **kw)  # the same object again, another rho
        fresh = _run_all(gpu, b, 57, 700, rho=2.0, objevals=1, **kw)
        assert not np.array_equal(first["xopt"], second["xopt"])
        for key in second:
            assert np.array_equal(second[key], fresh[key], equal_nan=True), key
        every = _run_all(gpu, b, 57, 700, rho=2.0, objevals=1, check_every=1, **kw)
        for key in fresh:
            assert np.array_equal(every[key], fresh[key], equal_nan=True), key
        plain = _run_all(gpu, b, 57, 700, rho=2.0, objevals=0, **kw)
        assert np.isnan(plain["objopt"]).all()
        for key in ("steps", "xopt", "zopt", "uopt", "pnorm", "perr", "Hnormsq"):
            assert np.array_equal(plain[key], fresh[key], equal_nan=True), key
    finally:
        a.close()
        b.close()


def test_refusals_through_the_c_abi(gpu, ap):
    L = ap._lib
    lib = L.load()
    rng = np.random.default_rng(0)

    def desc(m, n, K, ell=True):
        D = np.asfortranarray(rng.random((m, n)))
        E = np.asfortranarray(np.where(rng.random((m, max(K, 1))) < 0.5, 1.0, -1.0))
        d = L.SvmOvrDesc()
        lib.admm_svm_ovr_desc_default(C.byref(d))
        d.K, d.m, d.n, d.D, d.ldD, d.C = K, m, n, L.as_dp(D), m, 0.5
        if ell:
            d.ELL = L.as_dp(E)
        return d, (D, E)

    def refused(rc, code):
        assert rc == code, rc
        msg = lib.admm_last_error()
        assert msg and len(msg) > 0
        return msg.decode()

    h = C.c_void_p()
    d, keep = desc(500, 449, 2)
    assert "ADMM_PROB_LINEARSVM" in refused(lib.admm_svm_ovr_create(C.byref(d), C.byref(h)), L.E_UNSUPPORTED)
    assert not h.value
    d, keep = desc(64, 4, 0)
    refused(lib.admm_svm_ovr_create(C.byref(d), C.byref(h)), L.E_INVALID)
    d, keep = desc(64, 4, 2, ell=False)
    refused(lib.admm_svm_ovr_create(C.byref(d), C.byref(h)), L.E_INVALID)
    d, keep = desc(64, 4, 2)
    assert lib.admm_svm_ovr_create(C.byref(d), C.byref(h)) == L.OK
    try:
        for field, value in (("fast", L.FAST_STRONG), ("relax", 1.5), ("convtest", 1)):
            o = L.SvmOvrOptions()
            lib.admm_svm_ovr_options_default(C.byref(o))
            setattr(o, field, value)
            assert "ADMM_PROB_LINEARSVM" in refused(lib.admm_svm_ovr_run(h, C.byref(o), None, None), L.E_UNSUPPORTED)
    finally:
        lib.admm_svm_ovr_destroy(h)


def test_wide_problem_falls_back_to_one_engine_per_class(gpu):
    """n = 449: linearsvm_ovr still returns the per-class results"""
    p = gpu.synth.mnist_like_problem(seed=2, m=600, n=449)
    rng = np.random.default_rng(4)
    labels = rng.integers(0, 2, size=600).astype(np.float64)
    x0, z0, u0 = _starts(rng, 449, 600, 2)
    got = gpu.linearsvm_ovr(p["D"], labels, p["C"], dict(objevals=1, x0=x0, z0=z0, u0=u0))
    for c in range(2):
        ell = np.where(labels == c, 1.0, -1.0)
        ref = S.linearsvm(p["D"], ell, p["C"], dict(objevals=1, x0=x0[:, c], z0=z0[:, c], u0=u0[:, c]))
        assert got["steps"][c] == ref["steps"]
        _compare_class(got, c, ref, 1e-7)


def test_one_engine_stays_one_engine(gpu, digits):
    """after an OvR run in the same process the single-class solver still matches the oracle: no shared state"""
    d = digits
    gpu.linearsvm_ovr(d["D"], d["labels"], d["C"], dict(classes=[0.0, 1.0], x0=d["x0"][:, :2], z0=d["z0"][:, :2],
                                                        u0=d["u0"][:, :2]))
    p = gpu.synth.svm_problem(0)
    o = dict(objevals=1, x0=p["x0"], z0=p["z0"], u0=p["u0"])
    got = gpu.linearsvm(p["D"], p["ell"], p["C"], o)
    ref = S.linearsvm(p["D"], p["ell"], p["C"], o)
    assert got["steps"] == ref["steps"]
    for key in ("xvals", "zvals", "uvals", "pnorm", "perr", "objevals", "Hnormsq", "xopt", "zopt", "uopt"):
        _close(key, got[key], ref[key], 1e-7)
