"""Covariance selection, K fits in one run (csrc/covsel_multi.hip), on the device: every fit against the
oracle loop at its own (lambda, rho), the sizes of the one-workgroup path, more workgroups than CUs, the exact first
step, bit-equality of a fit alone and among others, reruns, agreement with the single-fit engine, symmetry, frozen
fits, the path and the refusals that need a device."""
import ctypes as C

import numpy as np
import pytest

import covsel_exact as ce
import covsel_multi_cases as cc
from covsel_restated import cov, samples
from test_gpu_covsel import SMALL_MAX, _SCALE, _close, _close_hist

pytestmark = pytest.mark.gpu

MAIN = (5, 256, 32)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same_bits(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), what


def _against_oracle(got, k, ref, dual=True, what=""):
    """fit k of a multi result against one oracle run: steps, iterates, every history entry, NaN past the last step"""
    s = int(ref["steps"])
    assert int(got["steps"][k]) == s, (what, k, int(got["steps"][k]), s)
    for key in ("xopt", "zopt", "uopt"):
        _close(got[key][:, :, k].reshape(-1, order="F"), ref[key], what=(what, k, key))
    hists = ["pnorm", "perr", "objevals"] + (["dnorm", "derr"] if dual else [])
    for key in hists:
        col = got[key][:, k]
        assert col.shape[0] >= s and np.all(np.isfinite(col[:s])), (what, k, key)
        assert np.all(np.isnan(col[s:])), (what, k, key)
        _close_hist(col[:s], np.asarray(ref[key])[:s], what=(what, k, key), scale=ref.get(_SCALE.get(key)))
    assert got["objopt"][k] == pytest.approx(float(ref["objevals"][s - 1]), rel=1e-9)
    if not dual:
        assert "dnorm" not in got and "derr" not in got


# ------------------------------------------------------------------------------------------------ parity with the oracle
@pytest.mark.parametrize("nodual", [0, 1])
@pytest.mark.parametrize("case", [MAIN, (11, 120, 24)], ids=["32", "24"])
def test_per_fit_parity(gpu, case, nodual):
    S = cc.case_S(case)
    lams = cc.grid(S)
    got = gpu.covarianceselection_multi(None, lams, dict(S=S, objevals=1, nodualerror=nodual))
    assert got["xopt"].shape == (case[2], case[2], 7)
    for k, lam in enumerate(lams):
        extra = dict(nodualerror=1) if nodual else {}
        _against_oracle(got, k, cc.oracle_fit(case, lam, 1.0, objevals=1, **extra), dual=not nodual, what=case)
    if not nodual:
        assert tuple(int(s) for s in got["steps"]) == cc.CASES[case]
    assert np.all(got["jacobi_sweeps"] >= got["steps"])


def test_per_fit_rho(gpu):
    S = cc.case_S(MAIN)
    lams = cc.grid(S)
    got = gpu.covarianceselection_multi(None, lams, dict(S=S, objevals=1, rho=cc.PER_FIT_RHO))
    assert np.array_equal(got["rhos"], np.array(cc.PER_FIT_RHO))
    for k, (lam, rho) in enumerate(zip(lams, cc.PER_FIT_RHO)):
        _against_oracle(got, k, cc.oracle_fit(MAIN, lam, rho, objevals=1), what="per-fit rho")
    assert len(set(int(s) for s in got["steps"])) >= 5


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 95, SMALL_MAX])
def test_sizes(gpu, n):
    S = cov(samples(20 + n, 4 * n + 8, n))
    lams = (0.05, 0.1, 0.3)
    opts = dict(objevals=1, maxiters=30, domaxiters=1)
    got = gpu.covarianceselection_multi(None, lams, dict(opts, S=S))
    assert np.all(got["steps"] == 30)
    for k, lam in enumerate(lams):
        _against_oracle(got, k, cc.oracle_fit(("size", n), lam, 1.0, S=S, **opts), what=n)


def test_more_workgroups_than_cus(gpu):
    S, lams = cc.many_case()
    assert lams.size == 300
    got = gpu.covarianceselection_multi(None, lams, dict(S=S, objevals=1))
    for k, lam in enumerate(lams):
        _against_oracle(got, k, cc.oracle_fit(cc.MANY_SAMPLES, lam, 1.0, objevals=1), what="K=300")
    assert len(set(int(s) for s in got["steps"])) > 8


# ------------------------------------------------------------------------------------------------ exact first step
REG = 0.1
RHOS = (2.0 ** -20, 1.0, 2.0 ** 20)


@pytest.mark.parametrize("n", [2, 16, 64, 95, SMALL_MAX])
@pytest.mark.parametrize("kind", ["range", "cluster", "zeros", "half-repeated", "equal"])
def test_first_step_exact(gpu, kind, n):
    s = ce.spectrum(kind, n, 100 + n)
    E = ce.Exact(s, 200 + n)
    S = E.S
    z = np.zeros((n, n, 3))
    got = gpu.covarianceselection_multi(None, [REG] * 3, dict(S=S, rho=RHOS, objevals=1, maxiters=1, z0=z, u0=z))
    assert np.all(got["steps"] == 1)
    lam = np.sort(-s)
    for k, rho in enumerate(RHOS):
        X, nld, trSX, _ = E.X(-s, rho)
        Xd = got["xopt"][:, :, k]
        _same_bits(Xd, Xd.T, "X symmetric")
        rx = ce.ratio(np.linalg.norm(Xd - X), ce.x_bound(lam, np.linalg.norm(S), np.linalg.norm(X), rho, n))
        print(f"\nRATIO first-step X n={n} {kind} rho={rho:g}: {rx:.3e}")
        assert rx <= 1.0, (rho, rx)
        Z = np.sign(X) * np.maximum(np.abs(X) - REG / rho, 0.0)
        obj = float(trSX) + float(nld) + REG * float(np.sum(np.abs(Z)))
        od = float(got["objevals"][0, k])
        assert np.isfinite(od)
        ro = ce.ratio(abs(od - obj), ce.first_obj_bound(S, X, lam, np.linalg.norm(S), rho, REG, n))
        print(f"RATIO first-step obj n={n} {kind} rho={rho:g}: {ro:.3e}")
        assert ro <= 1.0, (rho, od, obj, ro)


# ------------------------------------------------------------------------------------------------ bits
FIELDS = ("xopt", "zopt", "uopt", "pnorm", "perr", "dnorm", "derr", "objevals", "objopt", "steps", "jacobi_sweeps")


@pytest.fixture(scope="module")
def seven(gpu):
    """the K = 7 run of MAIN at the per-fit rhos, its object kept for a rerun"""
    S = cc.case_S(MAIN)
    lams = cc.grid(S)
    obj = gpu.CovselMulti(lams, S=S)
    run = lambda: obj.results(obj.run(rhos=np.array(cc.PER_FIT_RHO), objevals=1))
    first = run()
    yield dict(S=S, lams=lams, first=first, run=run)
    obj.close()


def _alone(gpu, S, lam, rho):
    obj = gpu.CovselMulti([lam], S=S)
    try:
        return obj.results(obj.run(rho=rho, objevals=1))
    finally:
        obj.close()


def test_alone_equals_together(gpu, seven):
    first = seven["first"]
    for k, (lam, rho) in enumerate(zip(seven["lams"], cc.PER_FIT_RHO)):
        one = _alone(gpu, seven["S"], lam, rho)
        s = int(one["steps"][0])
        for key in FIELDS:
            a, b = np.asarray(first[key]), np.asarray(one[key])
            if key in ("pnorm", "perr", "dnorm", "derr", "objevals"):
                _same_bits(a[:s, k], b[:, 0], (k, key))
            elif a.ndim == 3:
                _same_bits(a[:, :, k], b[:, :, 0], (k, key))
            else:
                _same_bits(np.asarray(a[k], dtype=np.float64), np.asarray(b[0], dtype=np.float64), (k, key))


def test_rerun_same_bits(seven):
    again = seven["run"]()
    for key in FIELDS:
        _same_bits(np.asarray(again[key], dtype=np.float64), np.asarray(seven["first"][key], dtype=np.float64), key)


def test_symmetric_in_bits(seven):
    for key in ("xopt", "zopt", "uopt"):
        for k in range(7):
            M = seven["first"][key][:, :, k]
            _same_bits(M, M.T, (key, k))


def test_frozen_fits(gpu, seven):
    """the fits stop at different steps: each history is NaN past its own last step, and the fit that stops first keeps
    the iterates it stopped with through every later launch"""
    first = seven["first"]
    steps = first["steps"]
    assert len(set(int(s) for s in steps)) >= 5
    S_max = int(steps.max())
    for key in ("pnorm", "perr", "dnorm", "derr", "objevals"):
        assert first[key].shape == (S_max, 7)
        for k in range(7):
            assert np.all(np.isfinite(first[key][:steps[k], k])) and np.all(np.isnan(first[key][steps[k]:, k])), (key, k)
    k = int(np.argmin(steps))
    assert S_max - int(steps[k]) > 8 * 2  # (several launches of check_every = 8 iterations follow its stop)
    one = _alone(gpu, seven["S"], seven["lams"][k], cc.PER_FIT_RHO[k])
    for key in ("xopt", "zopt", "uopt"):
        _same_bits(first[key][:, :, k], one[key][:, :, 0], key)


# ------------------------------------------------------------------------------------------------ the existing engine
def test_agrees_with_single_fit_engine(gpu):
    D = samples(*MAIN)
    lams = cc.grid(cc.case_S(MAIN))
    got = gpu.covarianceselection_multi(D, lams, dict(objevals=1))
    for k, lam in enumerate(lams):
        one = gpu.covarianceselection(D, float(lam), dict(objevals=1))
        assert int(got["steps"][k]) == int(one["steps"]), k
        for key in ("xopt", "zopt", "uopt"):
            _close(got[key][:, :, k], one[key], what=(k, key))
        s = int(one["steps"])
        for key in ("pnorm", "perr", "dnorm", "derr", "objevals"):
            _close_hist(got[key][:s, k], np.asarray(one[key])[:s], what=(k, key), scale=one.get(_SCALE.get(key)))


# ------------------------------------------------------------------------------------------------ the path
def test_path(gpu):
    D = samples(*MAIN)
    lmax = gpu.covarianceselection_lambda_max(D)
    assert lmax == pytest.approx(cc.lambda_max(cc.case_S(MAIN)), rel=1e-12)
    lams = 1.25 * lmax * np.logspace(0.0, -2.0, 7)
    res = gpu.covarianceselection_path(D, lams, dict(objevals=1))
    Z0 = res["zopt"][:, :, 0]
    assert np.array_equal(Z0, np.diag(np.diag(Z0)))
    assert res["df"][0] == 0 and np.all(np.diff(res["df"]) >= 0) and res["df"][-1] > 0
    assert [cc.df_of(res["zopt"][:, :, k]) for k in range(7)] == list(res["df"])
    auto = gpu.covarianceselection_path(D, None, dict(nlambda=4))
    assert auto["lams"].shape == (4,) and auto["lams"][0] == pytest.approx(lmax, rel=1e-12)
    assert auto["lams"][-1] == pytest.approx(1e-2 * lmax, rel=1e-12)


def test_pathtest_passes(gpu):
    results, test = gpu.testers.covarianceselectionpathtest(0)
    assert test["failed"] == 0, (test["diagonal_at_top"], test["df"], test["objopt"], test["trueobjopt"])
    assert test["diagonal_at_top"] and test["df_monotone"]


def test_S_in_place_of_D(gpu):
    D = samples(*MAIN)
    lams = cc.grid(cc.case_S(MAIN))[:3]
    obj = gpu.CovselMulti(lams, D=D)
    try:
        Sd = obj.cov()
        fromD = obj.results(obj.run(objevals=1))
    finally:
        obj.close()
    _same_bits(Sd, Sd.T, "COV symmetric")
    assert np.max(np.abs(Sd - np.cov(D, rowvar=False))) <= 1e-12 * np.max(np.abs(Sd))
    fromS = gpu.covarianceselection_multi(None, lams, dict(S=Sd, objevals=1))
    for key in FIELDS:
        _same_bits(np.asarray(fromD[key], dtype=np.float64), np.asarray(fromS[key], dtype=np.float64), key)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_on_the_device(gpu):
    L, lib = gpu._lib, gpu._lib.load()
    n = SMALL_MAX + 1
    S = np.asfortranarray(np.eye(n))
    lam = np.array([0.1])
    d = L.CovselMultiDesc()
    lib.admm_covsel_multi_desc_default(C.byref(d))
    d.K, d.n, d.S, d.lam = 1, n, L.as_dp(S), L.as_dp(lam)
    h = C.c_void_p()
    assert lib.admm_covsel_multi_create(C.byref(d), C.byref(h)) == L.E_UNSUPPORTED
    assert b"ADMM_PROB_COVSEL" in lib.admm_last_error() and not h.value
    with pytest.raises(gpu.AdmmError, match="ADMM_PROB_COVSEL") as ei:
        gpu.CovselMulti([0.1], S=S)
    assert ei.value.code == L.E_UNSUPPORTED
    S8 = cov(samples(13, 64, 8))
    obj = gpu.CovselMulti([0.1, 0.2], S=S8)
    try:
        with pytest.raises(ValueError, match="z0"):
            obj.run(z0=np.zeros((8, 8, 3)))
        with pytest.raises(ValueError, match="u0"):
            obj.run(u0=np.zeros((64, 1)))
        with pytest.raises(ValueError, match="rhos"):
            obj.run(rhos=[1.0])
        with pytest.raises(gpu.AdmmError, match="fit 1: rho") as ei:
            obj.run(rhos=[1.0, -1.0])
        assert ei.value.code == L.E_INVALID
        with pytest.raises(gpu.AdmmError, match="relaxation") as ei:
            obj.run(relax=1.5)
        assert ei.value.code == L.E_UNSUPPORTED
        assert np.all(obj.run(maxiters=5, domaxiters=1)["steps"] == 5)  # the object is still usable
    finally:
        obj.close()
    with pytest.raises(ValueError, match="z0"):
        gpu.covarianceselection_multi(None, [0.1, 0.2], dict(S=S8, z0=np.zeros((8, 8))))


def test_large_n_routes_to_the_engine(gpu):
    """n > 96: the fits run one after the other through the per-fit engine and the same keys come back"""
    n = SMALL_MAX + 4
    D = samples(31, 3 * n, n)
    lams = (0.2, 0.4)
    got = gpu.covarianceselection_multi(D, lams, dict(objevals=1, maxiters=12, domaxiters=1))
    assert got["xopt"].shape == (n, n, 2) and np.all(got["steps"] == 12)
    for k, lam in enumerate(lams):
        one = gpu.covarianceselection(D, lam, dict(objevals=1, maxiters=12, domaxiters=1))
        _close(got["xopt"][:, :, k], one["xopt"], what="xopt")
    for key in ("zopt", "uopt", "pnorm", "perr", "dnorm", "derr", "objevals", "objopt", "lams", "rhos",
                "jacobi_sweeps", "runtime", "solverruntime"):
        assert key in got, key
