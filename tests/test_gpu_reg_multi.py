"""Quantile / LAD / Huber regression, K fits in one pass over D, on the device: every fit against the
oracle's loop with the restated prox (tests/loss_restated.py) at the 1e-7 relative that test_gpu_loss holds the single
engine to, against the single engines themselves, chunking and freezing, re-runs, weights, warm starts, the refusals of
the C ABI, the quantile property and the launch counts.  The shapes are the pass kernel's edges (reg_multi_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import reg_multi_cases as Cs

pytestmark = pytest.mark.gpu

TOL = 1e-7  # tests/test_gpu_loss.py::_same_run: the single engine against the same restatement


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert not np.isnan(got).any() and not np.isnan(ref).any()
    return float(np.max(np.abs(got - ref)) / max(1e-300, np.max(np.abs(ref))))


def _multi(gpu, D, S, fits, w=None, **opts):
    o = dict(objevals=1, **opts)
    if w is not None:
        o["weights"] = w
    return gpu.robustfit_multi(D, S, list(fits), o)


# ------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("mode", Cs.MODES)
@pytest.mark.parametrize("shape", Cs.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_fit_against_the_restatement(gpu, shape, mode):
    """K = 7 fits in one run (LAD, tau = 0.1 and 0.9, epsilon = 0.3, Huber delta = 1, Huber delta = 0.25 with slopes
    (2, 0.5), a second LAD fit; 'weighted': shared weights with zeros on all of them) against loss_restated.run per fit:
    xopt, zopt, uopt, steps, and the pnorm / perr / objevals histories at 1e-7 relative.  No fit sits on a stop
    knife-edge: |pnorm - perr| / perr > 1e-4 at the restatement's last two iterations, so 1e-7 cannot move steps."""
    D, S, w = Cs.case(shape, mode)
    ref = Cs.reference(shape, mode)
    edge = Cs.knife_edge(ref)
    print(f"{shape} {mode}: reference steps {[int(r['steps']) for r in ref]}, knife-edge margin {edge:.3e}")
    assert edge > 1e-4
    got = _multi(gpu, D, S, Cs.FITS, w, maxiters=Cs.MAXITERS)
    assert not got["fallback"] and got["chunk"] == gpu.RegMulti.chunk()
    worst = 0.0
    for k, r in enumerate(ref):
        st = int(r["steps"])
        assert int(got["steps"][k]) == st, (k, got["steps"], st)
        for key in ("xopt", "zopt", "uopt"):
            worst = max(worst, _rel(got[key][:, k], r[key]))
        for key in ("pnorm", "perr", "objevals"):
            worst = max(worst, _rel(got[key][:st, k], r[key]))
            assert np.isnan(got[key][st:, k]).all()
        worst = max(worst, _rel([got["objopt"][k]], [r["objopt"]]))
    print(f"{shape} {mode}: worst relative error {worst:.3e} (bound {TOL:g})")
    assert worst < TOL
    assert len(set(int(v) for v in got["steps"])) > 1  # the fits stop at different step counts


# ------------------------------------------------------------------------------------------- 2. the single engines
def test_equals_the_single_engines(gpu):
    """each column against gpu.lad / gpu.huberfit with nodualerror = 1 at 1e-9 relative on xopt, equal steps: 600 x 120"""
    D, s = Cs.problem(600, 120, 21)
    got = _multi(gpu, D, s, Cs.FITS, maxiters=Cs.MAXITERS)
    worst = 0.0
    for k, fit in enumerate(Cs.FITS):
        loss = Cs.loss_of(fit)
        one = getattr(gpu, loss.kind)(D, s, dict(loss.options(), nodualerror=1, objevals=1, maxiters=Cs.MAXITERS))
        assert int(one["steps"]) == int(got["steps"][k]), (k, one["steps"], got["steps"])
        worst = max(worst, _rel(got["xopt"][:, k], one["xopt"]))
    print(f"600 x 120: worst relative error of xopt against the single engines {worst:.3e} (bound 1e-9)")
    assert worst < 1e-9


# ------------------------------------------------------------------------------------------- 3. chunking, freezing
def test_chunks_and_frozen_fits(gpu):
    """K = 2*Kc + 3 with fit 0 duplicated into the last chunk: bitwise equal columns; check_every = 1 and 64 agree bit
    for bit; a fit that stopped at step s has NaN history past s and the xopt of an independent run capped at s"""
    D, s = Cs.problem(300, 20, 22)
    Kc = gpu.RegMulti.chunk()
    K = 2 * Kc + 3
    taus = np.linspace(0.08, 0.92, K - 1)
    fits = [dict(kind="lad", tau=float(t)) for t in taus] + [dict(kind="lad", tau=float(taus[0]))]
    a = _multi(gpu, D, s, fits, maxiters=60, check_every=1)
    b = _multi(gpu, D, s, fits, maxiters=60, check_every=64)
    for key in ("xopt", "zopt", "uopt", "pnorm", "perr", "objevals", "objopt", "steps"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
        assert np.array_equal(a[key][..., 0], a[key][..., K - 1], equal_nan=True), key
    steps = a["steps"]
    assert steps.min() < steps.max(), steps  # some fit froze while others went on
    k = int(np.argmin(steps))
    sk = int(steps[k])
    assert np.isnan(a["pnorm"][sk:, k]).all() and not np.isnan(a["pnorm"][:sk, k]).any()
    alone = _multi(gpu, D, s, [fits[k]], maxiters=sk, domaxiters=1)
    assert int(alone["steps"][0]) == sk
    assert np.array_equal(alone["xopt"][:, 0], a["xopt"][:, k])
    assert np.array_equal(alone["zopt"][:, 0], a["zopt"][:, k])


# ------------------------------------------------------------------------------------------- 4. re-run, weights, starts
def _fetch_all(gpu, obj, m, n):
    L = gpu._lib
    return dict(x=obj.fetch(L.REGM_F_XOPT, n), z=obj.fetch(L.REGM_F_ZOPT, m), u=obj.fetch(L.REGM_F_UOPT, m))


def test_rerun_weights_and_warm_start(gpu):
    D, S, w = Cs.case((200, 57), "weighted")
    m, n = D.shape
    kinds = [0 if f["kind"] == "lad" else 1 for f in Cs.FITS]
    losses = [Cs.loss_of(f) for f in Cs.FITS]
    obj = gpu.RegMulti(D, S, kinds, [l.a for l in losses], [l.b for l in losses], [l.eps for l in losses],
                       [l.delta for l in losses])
    try:
        s1 = obj.run(maxiters=30, objevals=1)
        first = _fetch_all(gpu, obj, m, n)
        s2 = obj.run(maxiters=30, objevals=1)
        again = _fetch_all(gpu, obj, m, n)
        assert np.array_equal(s1["steps"], s2["steps"]) and np.array_equal(s1["objopt"], s2["objopt"])
        for key in first:
            assert np.array_equal(first[key], again[key]), key  # run twice: the same bits
        obj.set_weights(w)
        obj.run(maxiters=30, objevals=1)
        weighted = _fetch_all(gpu, obj, m, n)
        assert not np.array_equal(weighted["z"], first["z"])
        with pytest.raises(gpu.AdmmError) as ei:  # a refused call changes nothing
            obj.set_weights(np.r_[w[:-1], -1.0])
        assert ei.value.code == gpu._lib.E_INVALID
        obj.run(maxiters=30, objevals=1)
        still = _fetch_all(gpu, obj, m, n)
        for key in weighted:
            assert np.array_equal(weighted[key], still[key]), key
        obj.set_weights(None)
        obj.run(maxiters=30, objevals=1)
        back = _fetch_all(gpu, obj, m, n)
        for key in first:
            assert np.array_equal(first[key], back[key]), key  # set_weights(None): the first run bit for bit
        # a run split in two by a warm start equals the unsplit run
        obj.run(maxiters=20, domaxiters=1)
        whole = _fetch_all(gpu, obj, m, n)
        obj.run(maxiters=12, domaxiters=1)
        half = _fetch_all(gpu, obj, m, n)
        obj.run(maxiters=8, domaxiters=1, x0=half["x"], z0=half["z"], u0=half["u"])
        joined = _fetch_all(gpu, obj, m, n)
        worst = max(_rel(joined[key], whole[key]) for key in whole)
        print(f"warm start: worst relative difference {worst:.3e} (bound 1e-12)")
        assert worst < 1e-12
    finally:
        obj.close()


# ------------------------------------------------------------------------------------------- 5. refusals of the C ABI
def _create(gpu, D, S, K, keep, **fields):
    L = gpu._lib
    lib = L.load()
    D, S = np.asfortranarray(D), np.asfortranarray(S)
    d = L.RegMultiDesc()
    lib.admm_reg_multi_desc_default(C.byref(d))
    d.K, d.m, d.n = K, D.shape[0], D.shape[1]
    d.D, d.ldD, d.S, d.ns = L.as_dp(D), D.shape[0], L.as_dp(S), S.shape[1]
    keep.extend((D, S))
    for name, v in fields.items():
        if name == "kind":
            arr = np.ascontiguousarray(v, dtype=np.int32)
            d.kind = arr.ctypes.data_as(C.POINTER(C.c_int32))
        else:
            arr = np.ascontiguousarray(v, dtype=np.float64)
            setattr(d, name, L.as_dp(arr))
        keep.append(arr)
    h = C.c_void_p()
    rc = lib.admm_reg_multi_create(C.byref(d), C.byref(h))
    return rc, h


def test_refusals_leave_the_process_able_to_create(gpu):
    L = gpu._lib
    lib = L.load()
    rng = np.random.default_rng(5)
    D, s = Cs.problem(80, 6, 23)
    S = s.reshape(-1, 1)
    keep = []

    def good():
        rc, h = _create(gpu, D, S, 2, keep, kind=[0, 1])
        assert rc == L.OK and h.value
        return h

    def refused(code, rc_h, needle=None):
        rc, h = rc_h
        msg = lib.admm_last_error().decode()
        assert rc == code and not h.value, (rc, code, msg)
        if needle:
            assert needle in msg, msg
        lib.admm_reg_multi_destroy(good())

    wide = rng.standard_normal((460, 449))
    refused(L.E_UNSUPPORTED, _create(gpu, wide, rng.standard_normal((460, 1)), 1, keep))       # n = 449
    refused(L.E_UNSUPPORTED, _create(gpu, rng.standard_normal((5, 6)), np.ones((5, 1)), 1, keep))  # m < n
    refused(L.E_INVALID, _create(gpu, D, S, 2, keep, kind=[0, 2]), "fit 1")
    refused(L.E_INVALID, _create(gpu, D, S, 2, keep, a=[1.0, 0.0]), "fit 1")
    refused(L.E_INVALID, _create(gpu, D, S, 2, keep, kind=[0, 0], delta=[1.0, 0.5]), "fit 1")
    refused(L.E_INVALID, _create(gpu, D, S, 2, keep, kind=[1, 0], epsilon=[0.2, 0.0]), "fit 0")
    refused(L.E_INVALID, _create(gpu, D, S, 2, keep, b=[np.nan, 1.0]), "fit 0")
    twin = D.copy()
    twin[:, 3] = twin[:, 2]
    refused(L.E_NUMERIC, _create(gpu, twin, S, 1, keep))                                       # two identical columns
    h = good()
    try:
        for field, value in (("relax", 1.5), ("fast", L.FAST_STRONG), ("convtest", 1)):
            o = L.RegMultiOptions()
            lib.admm_reg_multi_options_default(C.byref(o))
            setattr(o, field, value)
            assert lib.admm_reg_multi_run(h, C.byref(o), None, None) == L.E_UNSUPPORTED, field
        w = np.ones(80)
        w[7] = np.nan
        assert lib.admm_reg_multi_set_weights(h, L.as_dp(w)) == L.E_INVALID
        o = L.RegMultiOptions()
        lib.admm_reg_multi_options_default(C.byref(o))
        summ = (L.RegMultiSummary * 2)()
        assert lib.admm_reg_multi_run(h, C.byref(o), summ, None) == L.OK  # and the object still runs
        assert summ[0].steps >= 1 and summ[1].steps >= 1
    finally:
        lib.admm_reg_multi_destroy(h)


# ------------------------------------------------------------------------------------------- 6. quantile property
def test_quantileregmultitest(gpu):
    test = gpu.testers.quantileregmultitest(seed=0)
    print(f"taus {test['taus']}: #(z<0) {test['negative']}, #(z==0) {test['zero']}, slack {test['slack']}, "
          f"steps {list(test['steps'])}")
    assert test["failed"] == 0


def test_wide_fallback(gpu):
    """n = 460 > 448: one lad / huberfit engine per fit with nodualerror = 1, fallback = True, the same fields"""
    D, s = Cs.problem(600, 460, 24)
    fits = [dict(kind="lad", tau=0.3), dict(kind="huber", delta=0.5)]
    got = gpu.robustfit_multi(D, s, fits, dict(maxiters=15, objevals=1))
    assert got["fallback"] is True and got["xopt"].shape == (460, 2) and got["zopt"].shape == (600, 2)
    one = gpu.lad(D, s, dict(tau=0.3, nodualerror=1, maxiters=15, objevals=1))
    two = gpu.huberfit(D, s, dict(delta=0.5, nodualerror=1, maxiters=15, objevals=1))
    for k, r in enumerate((one, two)):
        assert int(got["steps"][k]) == int(r["steps"])
        assert np.array_equal(got["xopt"][:, k], np.asarray(r["xopt"]).reshape(-1))
        assert np.array_equal(got["zopt"][:, k], np.asarray(r["zopt"]).reshape(-1))


# ------------------------------------------------------------------------------------------- 7. launch counts
def test_launch_counts(gpu):
    """an iteration is 1 x-solve + ceil(K / Kc) passes + 1 sum / finalize launch, for K = 1, Kc and Kc + 1"""
    D, s = Cs.problem(300, 20, 22)
    Kc = gpu.RegMulti.chunk()
    for K in (1, Kc, Kc + 1):
        taus = np.linspace(0.1, 0.9, K)
        obj = gpu.RegMulti(D, s, [0] * K, list(taus), list(1.0 - taus))
        try:
            obj.run(maxiters=16, domaxiters=1)
            c = obj.launches()
        finally:
            obj.close()
        assert c["iterations"] == 16 and c["finalize"] == 16, c
        assert c["passes"] == 16 * -(-K // Kc), c
        # one launch of the explicit map; where create's probe kept the triangular solves, a pair per fit and one copy
        assert c["xsolve"] == 16 * (1 if c["explicit_map"] else K + 1), c
