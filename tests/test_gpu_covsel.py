"""Covariance selection on the device against the oracle loop driven by the restated reference closures
(tests/covsel_restated.py): per-iteration parity, both eigen-step paths, the loop variants, hard spectra, exact
symmetry, cov(D) on the device, engine reuse, the tester and the refusals."""
import numpy as np
import pytest

from covsel_restated import cov, oracle_run, samples

pytestmark = pytest.mark.gpu

SMALL_MAX = 96  # csrc/covsel.h: kCovselSmallMax, the last n of the one-workgroup path


def _run(ap, S, lam, options, D=None):
    args = {"lambda": lam}
    if D is None:
        args["S"] = S
    else:
        args["D"] = D
    minx, minz, _ = ap.getproxops("covarianceselection", args)
    n = S.shape[0]
    o = dict(options, A=1, B=-1, c=0, m=n, nA=n, nB=n)
    return ap.admm(minx, minz, o)


def _close(a, b, rtol=1e-9, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(np.linalg.norm(b), 1e-300)
    assert np.linalg.norm(a - b) <= rtol * scale, (what, np.linalg.norm(a - b) / scale)


def _close_hist(a, b, rtol=1e-9, what="", scale=None):
    # elementwise, with an absolute floor: 1e-3 of the history's largest value, or per iteration the size of what the
    # value is a difference of (`scale`: the residual norms cancel down from the iterates' size, which perr / derr carry)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    floor = 1e-3 * np.max(np.abs(b)) if b.size else 0.0
    if scale is not None:
        floor = np.maximum(floor, np.abs(np.asarray(scale, dtype=np.float64)))
    err = np.abs(a - b) / np.maximum(np.maximum(np.abs(b), floor), 1e-300)
    assert np.all(err <= rtol), (what, float(np.max(err)), int(np.argmax(err)))


def _compare(got, ref, keys=("xvals", "zvals", "uvals"), hists=("pnorm", "dnorm", "perr", "derr")):
    for k in ("steps", "convtest_failed_at"):  # (a convtest abort returns no steps: admm.m:692-701, q4)
        assert got.get(k) == ref.get(k), (k, got.get(k), ref.get(k))
    for k in keys:
        _close(got[k], ref[k], what=k)
    for k in hists:
        _close_hist(got[k], ref[k], what=k, scale=ref.get(_SCALE.get(k)))


_SCALE = {"pnorm": "perr", "dnorm": "derr"}


@pytest.mark.parametrize("lam", [0.05, 1.0])
@pytest.mark.parametrize("rho", [0.1, 1.0, 10.0])
def test_per_iteration_parity(gpu, lam, rho):
    D = samples(11, 512, 64)
    S = cov(D)
    opts = dict(rho=rho, objevals=1, stopcond="both", maxiters=400)
    got = _run(gpu, S, lam, opts)
    ref = oracle_run(S, lam, opts)
    _compare(got, ref, hists=("pnorm", "dnorm", "perr", "derr", "Hnormsq", "objevals"))
    assert got["objopt"] == pytest.approx(ref["objopt"], rel=1e-9)
    _close(got["xopt"], ref["xopt"], what="xopt")


@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, SMALL_MAX + 1, 300])
def test_sizes_on_both_paths(gpu, n):
    D = samples(20 + n, 4 * n + 8, n)
    S = cov(D)
    opts = dict(rho=1.0, objevals=1, maxiters=30, domaxiters=1)
    got = _run(gpu, S, 0.1, opts)
    ref = oracle_run(S, 0.1, opts)
    _compare(got, ref)
    _close_hist(got["objevals"], ref["objevals"], what="objevals")
    assert got["engine_info"]["jacobi_sweeps"] >= (1 if n > 1 else 0)


@pytest.mark.parametrize("variant", [dict(relax=1.6), dict(fast=1, fasttype="weak"), dict(fast=1, fasttype="strong"),
                                     dict(stopcond="hnorm"), dict(stopcond="both"), dict(record_history=0),
                                     dict(convtest=1), dict(check_every=3)],
                         ids=["relax", "fast-weak", "fast-strong", "hnorm", "both", "nohist", "convtest", "check3"])
def test_loop_variants(gpu, variant):
    D = samples(5, 256, 32)
    S = cov(D)
    opts = dict(variant, rho=1.0, objevals=1, maxiters=300)
    got = _run(gpu, S, 0.2, opts)
    ref = oracle_run(S, 0.2, opts)
    assert got.get("convtest_failed_at") == ref.get("convtest_failed_at")
    assert got.get("steps") == ref.get("steps")
    if variant.get("record_history", 1):
        for k in ("xvals", "zvals", "uvals"):
            _close(got[k], ref[k], what=k)
    for k in ("xopt", "zopt", "uopt"):
        assert (k in got) == (k in ref)
        if k in ref:
            _close(got[k], ref[k], what=k)
    hists = ["objevals"] + (["pnorm", "dnorm", "perr", "derr"] if variant.get("fasttype") != "weak" else [])
    if "stopcond" in variant or "convtest" in variant:
        hists.append("Hnormsq")
    for k in hists:
        _close_hist(got[k], ref[k], what=k, scale=ref.get(_SCALE.get(k)))
    if variant.get("fasttype") == "weak":
        # accelerated ADMM restarts when d > 0.999*dprev (admm.m:572-591): once d is rounding noise of the converged
        # iterate the decision is a coin toss of the last bits in the reference itself (tests/sweeps/fuzz_solvers.py:
        # knife_edge); the decisions and alphas must agree up to there
        ra, rb = np.asarray(got["restarted"]), np.asarray(ref["restarted"])
        bad = np.nonzero(ra != rb)[0]
        cut = int(bad[0]) if bad.size else ra.size
        if bad.size:
            noise = 1e-18 * max(1.0, float(np.max(np.abs(ref["xopt"]))) ** 2)
            assert max(got["dvals"][cut], ref["dvals"][cut]) <= noise, (cut, got["dvals"][cut], ref["dvals"][cut])
        _close_hist(got["avals"][:cut], ref["avals"][:cut], what="avals")


@pytest.mark.parametrize("case", ["identity", "rank-deficient", "rho-small", "rho-large"])
def test_hard_spectra(gpu, case):
    n = 64
    if case == "identity":
        S, rho = np.eye(n), 1.0  # M = -I: exactly diagonal, all eigenvalues equal, in the first iteration
    elif case == "rank-deficient":
        S, rho = cov(samples(6, 32, n)), 1.0  # rank 31: eigenvalue 0 repeated 33 times
    else:
        S, rho = cov(samples(7, 512, n)), (1e-3 if case == "rho-small" else 1e3)
    opts = dict(rho=rho, maxiters=60, domaxiters=1)
    got = _run(gpu, S, 0.1, opts)
    ref = oracle_run(S, 0.1, opts)
    _compare(got, ref)


@pytest.mark.parametrize("n", [40, SMALL_MAX + 3])
def test_iterates_exactly_symmetric(gpu, n):
    D = samples(8, 8 * n, n)
    res = gpu.covarianceselection(D, 0.3, dict(maxiters=50))
    for k in ("xopt", "zopt", "uopt"):
        M = res[k]
        assert M.shape == (n, n)
        assert np.array_equal(M, M.T), k
    X = res["xvals"][:, -1].reshape((n, n), order="F")
    assert np.array_equal(X, X.T)


def test_device_cov_and_the_solver(gpu):
    for mean in (0.0, 1e3):
        D = samples(9, 300, 48, mean=mean)
        minx, _, _ = gpu.getproxops("covarianceselection", {"D": D, "lambda": 1.0})
        Sd = minx.problem.engine.fetch(gpu._lib.F_COVSEL_S, 48 * 48, (48, 48))
        Sn = np.cov(D, rowvar=False)
        assert np.array_equal(Sd, Sd.T)
        assert np.max(np.abs(Sd - Sn)) <= 1e-12 * np.max(np.abs(Sn)), mean
        minx.problem.engine.close()
    D = samples(10, 300, 48, mean=1e3)
    opts = dict(objevals=1)
    got = gpu.covarianceselection(D, 0.5, dict(opts))
    ref = oracle_run(cov(D), 0.5, dict(opts))
    _compare(got, ref)
    _close(got["xopt"], ref["xopt"].reshape((48, 48), order="F"), what="xopt")
    assert "solverruntime" in got


def test_engine_reuse_is_stateless(gpu):
    D = samples(12, 512, 64)
    S = cov(D)
    minx, minz, _ = gpu.getproxops("covarianceselection", {"S": S, "lambda": 0.3})
    o = dict(A=1, B=-1, c=0, m=64, nA=64, nB=64, objevals=1, maxiters=200)
    first = gpu.admm(minx, minz, dict(o, rho=1.0))
    other = gpu.admm(minx, minz, dict(o, rho=2.0))
    again = gpu.admm(minx, minz, dict(o, rho=1.0))
    fresh2 = _run(gpu, S, 0.3, dict(objevals=1, maxiters=200, rho=2.0))
    for a, b in ((again, first), (other, fresh2)):
        assert a["steps"] == b["steps"]
        for k in ("xvals", "zvals", "uvals", "objevals", "pnorm", "dnorm"):
            _close(a[k], b[k], what=k)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_tester_passes(gpu, seed):
    results, test = gpu.testers.covarianceselectiontest(seed)
    assert test["failed"] == 0, (test["objopt"], test["trueobjopt"])
    assert results["steps"] >= 1


def test_refusals(gpu):
    S = cov(samples(13, 64, 8))
    with pytest.raises(ValueError, match="square"):
        gpu.getproxops("covarianceselection", {"S": S[:, :7], "lambda": 1.0})
    bad = S.copy()
    bad[0, 1] += 1e-6
    with pytest.raises(gpu.AdmmError, match="symmetric") as ei:
        gpu.getproxops("covarianceselection", {"S": bad, "lambda": 1.0})
    assert ei.value.code == gpu._lib.E_INVALID
    for lam in (0.0, -1.0):
        with pytest.raises(gpu.AdmmError, match="lambda") as ei:
            gpu.getproxops("covarianceselection", {"S": S, "lambda": lam})
        assert ei.value.code == gpu._lib.E_INVALID
    with pytest.raises(gpu.AdmmError, match="xsolve") as ei:
        gpu.getproxops("covarianceselection", {"S": S, "lambda": 1.0, "xsolve": "cg"})
    assert ei.value.code == gpu._lib.E_UNSUPPORTED
    minx, minz, _ = gpu.getproxops("covarianceselection", {"S": S, "lambda": 1.0})
    o = dict(A=1, B=-1, c=0, m=8, nA=8, nB=8, maxiters=5)
    with pytest.raises(NotImplementedError, match="covarianceselection"):
        gpu.admm(minx, lambda x, z, u, rho: x + u, o)
    with pytest.raises(gpu.AdmmError) as ei:
        minx.problem.engine.set_callbacks(zmin=lambda x, z, u, rho: x + u)
    assert ei.value.code == gpu._lib.E_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="adaptive"):
        gpu.admm(minx, minz, dict(o, adaptive=1, convtest=1))
    assert gpu.admm(minx, minz, o)["steps"] == 5  # the engine is still usable
