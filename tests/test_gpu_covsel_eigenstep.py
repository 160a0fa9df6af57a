"""The covariance-selection eigen-step (csrc/covsel.hip) against the exact reference of tests/covsel_exact.py, not
against the restatement: the first x-update on matrices with an exactly known spectrum, every x-update of a run held
in isolation to the stated bound (both paths, the loop variants, long runs for warm-start drift), the large path's
loop variants against the oracle, the lower-triangle semantics, cov(D) at its edges and graph replay."""
import math

import numpy as np
import pytest

import covsel_exact as ce
from covsel_restated import cov, oracle_run, samples
from test_gpu_covsel import SMALL_MAX, _SCALE, _close, _close_hist, _run

pytestmark = pytest.mark.gpu

REG = 0.1  # the l1 weight (lambda) of the first-step cases


def _report(what, r):
    print(f"\nRATIO {what}: {r:.3e}")


# ------------------------------------------------------------------------------------------------ first x-update
# (n, spectrum of S, rho): a covering subset of sizes x spectra x rho; M_1 = -S exactly (z0 = u0 = 0)
FIRST = [
    (1, "mixed", 1.0),
    (2, "range", 2.0 ** -20),
    (4, "equal", 2.0 ** 20),
    (16, "cluster", 1.0),
    (64, "half-repeated", 2.0 ** -20),
    (95, "zeros", 1.0),
    (96, "range", 1.0),
    (96, "cluster", 2.0 ** 20),
    (97, "mixed", 2.0 ** 20),
    (98, "cluster", 2.0 ** -20),
    (129, "zeros", 2.0 ** -20),  # det X = 2^(>1280): overflows fp64
    (256, "zeros", 2.0 ** 20),  # det X = 2^(-2560): underflows
    (256, "half-repeated", 1.0),
    (300, "range", 2.0 ** -20),
    (300, "equal", 1.0),
    (1024, "mixed", 1.0),
]


@pytest.mark.parametrize("n,kind,rho", FIRST, ids=[f"{n}-{k}-{r:g}" for n, k, r in FIRST])
def test_first_x_update_exact(gpu, n, kind, rho):
    s = ce.spectrum(kind, n, 100 + n)
    E = ce.Exact(s, 200 + n)
    S = E.S
    X, nld, trSX, _ = E.X(-s, rho)
    got = _run(gpu, S, REG, dict(rho=rho, objevals=1, maxiters=1))
    assert got["steps"] == 1
    Xd = got["xvals"][:, 0].reshape((n, n), order="F")
    assert np.array_equal(Xd, Xd.T)
    lam = np.sort(-s)
    bx = ce.x_bound(lam, np.linalg.norm(S), np.linalg.norm(X), rho, n)
    rx = ce.ratio(np.linalg.norm(Xd - X), bx)
    _report(f"first-step X n={n} {kind} rho={rho:g}", rx)
    assert rx <= 1.0, rx
    # objevals[0] = trace(S X) - log det X + lambda ||Z||_1, Z = soft(X, lambda / rho): from the exact X
    Z = np.sign(X) * np.maximum(np.abs(X) - REG / rho, 0.0)
    obj = float(trSX) + float(nld) + REG * float(np.sum(np.abs(Z)))
    od = float(got["objevals"][0])
    assert np.isfinite(od)  # q27: the device never forms det X
    ro = ce.ratio(abs(od - obj), ce.first_obj_bound(S, X, lam, np.linalg.norm(S), rho, REG, n))
    _report(f"first-step obj n={n} {kind} rho={rho:g}", ro)
    assert ro <= 1.0, (od, obj, ro)


def test_first_x_update_logdet_alone(gpu):
    """With S = 0 the objective is -log det X + lambda ||Z||_1 exactly: the log-determinant is not hidden behind a
    large trace term.  f(0) = 1/sqrt(rho) on both sides of fp64's det range."""
    for n, rho in ((24, 2.0 ** -20), (160, 2.0 ** -20), (160, 2.0 ** 20)):
        got = _run(gpu, np.zeros((n, n)), REG, dict(rho=rho, objevals=1, maxiters=1))
        Xd = got["xvals"][:, 0].reshape((n, n), order="F")
        f0 = rho ** -0.5
        np.testing.assert_array_equal(Xd, np.eye(n) * f0)
        obj = n * np.log(rho) / 2 + REG * n * max(f0 - REG / rho, 0.0)
        assert got["objevals"][0] == pytest.approx(obj, rel=4 * n * ce.EPS), (n, rho)


# ------------------------------------------------------------------------------------------------ x-updates in isolation
def _isolated(res, S, rho, fast, ks):
    """max over k in ks of ||X_k - f(M_k)||_F / bound, M_k = rho (Z_{k-1} - U_{k-1}) - S rebuilt from the device's own
    history (V_{k-1} - Uhat_{k-1} under fast ADMM; Z_0 = U_0 = 0)."""
    n = S.shape[0]
    zk, uk = ("vvals", "uhatvals") if fast else ("zvals", "uvals")
    worst = 0.0
    for k in ks:
        y = np.zeros(n * n) if k == 0 else res[zk][:, k - 1] - res[uk][:, k - 1]
        M = rho * y.reshape((n, n), order="F") - S
        Xr, lam = ce.x_ref(M, rho)
        Xd = res["xvals"][:, k].reshape((n, n), order="F")
        b = ce.x_bound(lam, np.linalg.norm(np.tril(M) + np.tril(M, -1).T), np.linalg.norm(Xr), rho, n)
        worst = max(worst, ce.ratio(np.linalg.norm(Xd - Xr), b))
    return worst


VARIANTS = {"plain": {}, "relax": dict(relax=1.6), "fast-strong": dict(fast=1, fasttype="strong"),
            "fast-weak": dict(fast=1, fasttype="weak")}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n", [32, 110])
def test_every_x_update_in_isolation(gpu, n, variant):
    S = cov(samples(30 + n, 4 * n, n))
    rho = 1.0
    v = VARIANTS[variant]
    res = _run(gpu, S, 0.2, dict(v, rho=rho, maxiters=120, domaxiters=1))
    assert res["steps"] == 120
    r = _isolated(res, S, rho, "fast" in v, range(res["steps"]))
    _report(f"isolated n={n} {variant}", r)
    assert r <= 1.0, r


@pytest.mark.parametrize("n", [48, 100])
def test_long_run_warm_start_drift(gpu, n):
    """1500 x-updates from one basis, each warm-started from the last: the late ones are held to the same bound."""
    S = cov(samples(40 + n, 2 * n, n))
    rho, N = 30.0, 1500  # a large rho: Z and U move slowly, so every x-update still rotates
    res = _run(gpu, S, 0.05, dict(rho=rho, maxiters=N, domaxiters=1))
    assert res["steps"] == N
    sweeps = res["engine_info"]["jacobi_sweeps"] / N
    # the same run cut 100 iterations short (same trajectory): the difference is the sweeps of the last 100 x-updates
    head = _run(gpu, S, 0.05, dict(rho=rho, maxiters=N - 100, domaxiters=1))["engine_info"]
    late_sweeps = (res["engine_info"]["jacobi_sweeps"] - head["jacobi_sweeps"]) / 100
    early = _isolated(res, S, rho, False, range(0, 100, 5))
    late = _isolated(res, S, rho, False, range(N - 100, N, 5))
    _report(f"long run n={n} early", early)
    _report(f"long run n={n} late", late)
    print(f"SWEEPS long run n={n}: {sweeps:.2f} per x-update, {late_sweeps:.2f} in the last 100")
    # an x-update that rotates nothing takes exactly one sweep: the run as a whole rotates well beyond that, and x-updates
    # late in the run still rotate
    assert sweeps > 2.5, sweeps
    assert late_sweeps > 1.5, late_sweeps
    assert max(early, late) <= 1.0, (early, late)


# ------------------------------------------------------------------------------------------------ large-path loop
@pytest.mark.parametrize("variant", [dict(relax=1.6), dict(fast=1, fasttype="weak"), dict(fast=1, fasttype="strong"),
                                     dict(stopcond="hnorm"), dict(stopcond="both"), dict(record_history=0),
                                     dict(convtest=1), dict(check_every=3)],
                         ids=["relax", "fast-weak", "fast-strong", "hnorm", "both", "nohist", "convtest", "check3"])
def test_loop_variants_large_path(gpu, variant):
    n = 110
    assert n > SMALL_MAX
    S = cov(samples(6, 4 * n, n))  # converges at step 28: inside a batch of three
    opts = dict(variant, rho=1.0, objevals=1, maxiters=301)
    got = _run(gpu, S, 0.2, opts)
    ref = oracle_run(S, 0.2, opts)
    assert got.get("convtest_failed_at") == ref.get("convtest_failed_at")
    assert got.get("steps") == ref.get("steps")
    if "check_every" in variant:
        assert ref["steps"] % 3 != 0, ref["steps"]  # the stop lands inside a batch of three
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
    if variant.get("fasttype") == "weak":  # (the restart decisions: as test_gpu_covsel.test_loop_variants)
        ra, rb = np.asarray(got["restarted"]), np.asarray(ref["restarted"])
        bad = np.nonzero(ra != rb)[0]
        cut = int(bad[0]) if bad.size else ra.size
        if bad.size:
            noise = 1e-18 * max(1.0, float(np.max(np.abs(ref["xopt"]))) ** 2)
            assert max(got["dvals"][cut], ref["dvals"][cut]) <= noise, (cut, got["dvals"][cut], ref["dvals"][cut])
        _close_hist(got["avals"][:cut], ref["avals"][:cut], what="avals")


# ------------------------------------------------------------------------------------------------ lower triangle
@pytest.mark.parametrize("n", [12, 100])
def test_lower_triangle_semantics(gpu, n):
    s = ce.spectrum("mixed", n, 7)
    E = ce.Exact(s, 8)
    S = E.S
    rho = 1.0
    X, nld, trSX, _ = E.X(-s, rho)
    # the engine accepts |S - S'| <= 1e-12 max|S|: use all of it, above the diagonal only, with the signs of X there
    # (the largest change of trace(S X) the tolerance allows)
    dS = np.triu(np.where(X >= 0, 1.0, -1.0), 1) * (1e-12 * (1 - 1e-3)) * np.max(np.abs(S))
    Su = S + dS
    assert np.array_equal(np.tril(Su), np.tril(S))
    opts = dict(rho=rho, objevals=1, maxiters=1)
    base = _run(gpu, S, REG, dict(opts))
    got = _run(gpu, Su, REG, dict(opts))
    # X is f of the mirrored lower triangle: M_1 = -tril(Su) mirrored = -S, so X is the same, bit for bit
    Xd = got["xvals"][:, 0].reshape((n, n), order="F")
    np.testing.assert_array_equal(got["xvals"], base["xvals"])
    lam = np.sort(-s)
    r = ce.ratio(np.linalg.norm(Xd - X), ce.x_bound(lam, np.linalg.norm(S), np.linalg.norm(X), rho, n))
    _report(f"lower-triangle X n={n}", r)
    assert r <= 1.0, r
    # the trace term weighs X by the full S, upper triangle included: with X, Z and -log det X the same in both runs,
    # the objectives differ by sum(triu(Su - S, 1) .* X).  Held to the rounding of the two n^2-term sums (each lane
    # adds <= ceil(n^2 / 256) terms, then a 256-lane tree and a block sum of <= 1024 partials: depth <= that + 40) and
    # of the objective's three-term total
    want = math.fsum((dS * Xd).ravel())
    Z = np.sign(Xd) * np.maximum(np.abs(Xd) - REG / rho, 0.0)
    depth = math.ceil(n * n / 256) + 40
    bound = (2 * ce.C * depth * ce.EPS * float(np.sum(np.abs(Su * Xd)))
             + 4 * ce.EPS * (abs(float(trSX)) + abs(float(nld)) + REG * float(np.sum(np.abs(Z)))))
    assert abs(want) >= 3 * bound  # a trace from the mirrored lower triangle (a difference of 0) would fail below
    diff = float(got["objevals"][0]) - float(base["objevals"][0])
    ro = ce.ratio(abs(diff - want), bound)
    _report(f"lower-triangle obj n={n}", ro)
    assert ro <= 1.0, (diff, want, ro)


# ------------------------------------------------------------------------------------------------ cov(D)
@pytest.mark.parametrize("m,n,mean", [(2, 5, 0.0), (20, 64, 0.0), (1001, 130, 0.0), (400, 40, 1e8)],
                         ids=["m2", "rank-deficient", "padded", "mean1e8"])
def test_device_cov_edges(gpu, m, n, mean):
    D = samples(50 + m, m, n, mean=mean)
    minx, _, _ = gpu.getproxops("covarianceselection", {"D": D, "lambda": 1.0})
    try:
        Sd = minx.problem.engine.fetch(gpu._lib.F_COVSEL_S, n * n, (n, n))
    finally:
        minx.problem.engine.close()
    assert np.array_equal(Sd, Sd.T)
    Sr, A = ce.cov_ref(D)
    B = ce.cov_bound(D, A)
    err = np.abs(Sd - np.asarray(Sr, dtype=np.float64))
    _report(f"cov m={m} n={n} mean={mean:g}", float(np.max(err / B)))
    assert np.all(err <= B), float(np.max(err / B))


# ------------------------------------------------------------------------------------------------ graph replay
@pytest.mark.parametrize("n", [32, 110])
def test_graph_replay_matches_eager(gpu, monkeypatch, n):
    S = cov(samples(60 + n, 4 * n, n))
    opts = dict(rho=1.0, objevals=1, maxiters=80)
    monkeypatch.delenv("ADMM_HIP_GRAPH", raising=False)
    eager = _run(gpu, S, 0.2, dict(opts))
    monkeypatch.setenv("ADMM_HIP_GRAPH", "1")
    graph = _run(gpu, S, 0.2, dict(opts))
    assert graph["steps"] == eager["steps"]
    for k in ("xvals", "zvals", "uvals", "objevals", "pnorm", "dnorm"):
        np.testing.assert_array_equal(graph[k], eager[k], err_msg=k)  # same kernels, same order: bitwise
