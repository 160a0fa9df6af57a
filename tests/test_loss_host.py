"""The loss family of the LAD and Huber engines on the CPU: the restated prox (tests/loss_restated.py)
against the subgradient condition of its own minimisation, against the oracle's formulas at the defaults and against the
quantile-regression linear programme, and what the binding layer and the Python surfaces refuse before any device work."""
import numpy as np
import pytest
import scipy.optimize as sopt

import loss_restated as R
from oracle import proxops_ref

EPS = R.EPS


# ------------------------------------------------------------------------------------ (a) the subgradient condition
def _members():
    w = np.random.default_rng(5).uniform(0.5, 2.0, 400)
    w[7] = 0.0
    return {
        "lad": R.Loss("lad"),
        "quantile": R.Loss("lad", slopes=(0.9, 0.1)),
        "quantile-weights": R.Loss("lad", weights=w, slopes=(0.2, 0.8)),
        "svr": R.Loss("lad", epsilon=0.3),
        "svr-asym-weights": R.Loss("lad", weights=w, slopes=(1.5, 0.25), epsilon=0.7),
        "huber": R.Loss("huberfit"),
        "huber-delta": R.Loss("huberfit", delta=0.5),
        "huber-asym-weights": R.Loss("huberfit", weights=w, slopes=(1.5, 0.5), delta=2.5),
    }


@pytest.mark.parametrize("rho", [0.05, 1.0, 37.0])
@pytest.mark.parametrize("name", list(_members()))
def test_prox_satisfies_the_subgradient_condition(name, rho):
    """0 in w*dphi(z) + rho*(z - v) at z = prox(v), for v in every branch and exactly on every breakpoint (of every
    element's own weight); every branch must be met.  The residual of the condition is measured against the sizes that
    enter it."""
    loss = _members()[name]
    n = 400
    v = R.breakpoint_vector(loss, rho, n=n)
    z = R.prox(v, loss, rho)
    w = np.ones(n) if loss.w is None else loss.w
    lo, hi = R.dphi_interval(z, loss)
    g = rho * (v - z)  # must lie in w*[lo, hi]
    tol = 16 * EPS * (rho * (np.abs(v) + np.abs(z)) + w * max(loss.a, loss.b) * max(1.0, loss.delta))
    assert np.all(g >= w * lo - tol) and np.all(g <= w * hi + tol), name
    # a zero weight returns v bit for bit
    assert np.array_equal(z[w == 0], v[w == 0])
    if loss.kind == "lad":
        ta, tb = (w * loss.a) / rho, (w * loss.b) / rho
        branches = [v > loss.eps + ta, (v >= loss.eps) & (v <= loss.eps + ta), (v > -loss.eps) & (v < loss.eps),
                    (v >= -loss.eps - tb) & (v <= -loss.eps), v < -loss.eps - tb]
        if loss.eps == 0:
            branches.pop(2)
        assert all(b.any() for b in branches)
        dead = (v > -loss.eps) & (v < loss.eps)
        assert np.array_equal(z[dead], v[dead])  # the dead zone returns v bit for bit
        flat_hi = (v >= loss.eps) & (v <= loss.eps + ta) & (w > 0)
        flat_lo = (v >= -loss.eps - tb) & (v <= -loss.eps) & (w > 0) & ~flat_hi
        assert np.all(z[flat_hi] == loss.eps) and np.all(z[flat_lo] == -loss.eps)  # the flats land on +-eps exactly
    else:
        assert (np.abs(z) > loss.delta).any() and (np.abs(z) < loss.delta).any() and (v < 0).any() and (v > 0).any()


# ------------------------------------------------------------------------------------ (b) the defaults
def test_defaults_are_the_oracle_s_formulas():
    v = np.random.default_rng(6).standard_normal(2000) * 3.0
    v[:4] = (0.0, 1.0, -1.0, 0.5)
    for rho in (0.05, 1.0, 37.0):
        lad = R.prox(v, R.Loss("lad"), rho)
        ref = proxops_ref.soft_threshold(v, 1.0 / rho)
        assert np.max(np.abs(lad - ref)) <= 2 * EPS * np.max(np.abs(v))
        hub = R.prox(v, R.Loss("huberfit"), rho)
        refh = 1.0 / (1.0 + rho) * (rho * v + proxops_ref.soft_threshold(v, 1.0 + 1.0 / rho))  # getProxOps.m:1529-1539
        assert np.max(np.abs(hub - refh)) <= 8 * EPS * np.max(np.abs(v))
    z = v.copy()
    assert abs(R.g_of(z, R.Loss("lad")) - np.sum(np.abs(z))) <= 1e-12
    cvx = np.where(np.abs(z) <= 1.0, z * z, 2.0 * np.abs(z) - 1.0)
    assert abs(R.g_of(z, R.Loss("huberfit")) - 0.5 * np.sum(cvx)) <= 1e-12


# ------------------------------------------------------------------------------------ (c), (d) quantile regression
def _quantile_lp(D, s, a, b):
    """min a*sum(p) + b*sum(q) s.t. D*x - s = p - q, p, q >= 0 (HiGHS)"""
    m, n = D.shape
    c = np.r_[np.zeros(n), a * np.ones(m), b * np.ones(m)]
    res = sopt.linprog(c, A_eq=np.hstack([D, -np.eye(m), np.eye(m)]), b_eq=s,
                       bounds=[(None, None)] * n + [(0, None)] * (2 * m), method="highs")
    assert res.status == 0, res.message
    return float(res.fun), res.x[:n]


@pytest.fixture(scope="module")
def quantile_runs(ap):
    D, s = R.regression(ap.synth, 200, 8, 0)
    runs = {tau: R.run("lad", D, s, R.Loss("lad", slopes=(tau, 1.0 - tau)), dict(objevals=1)) for tau in (0.1, 0.5, 0.9)}
    return D, s, runs


MEASURED_GAP = 2.91e-6  # the largest |objopt - LP| / LP of the three runs below (tau = 0.1)


@pytest.mark.parametrize("tau", [0.1, 0.5, 0.9])
def test_quantile_run_against_the_linear_programme(ap, quantile_runs, tau):
    """The restated run stops at the default tolerances (here: at maxiters = 1000), not at the optimum.  Measured on
    the CPU at 200 x 8, seed 0: (objopt - LP)/LP = +2.90e-6 (tau = 0.1), -1.94e-6 (0.5), -4.8e-7 (0.9) -- objopt is g(z)
    of an infeasible pair, so it may lie below the optimum -- and the count condition #(z < 0) <= tau*m <= #(z < 0) +
    #(z == 0) holds with slack 0 (16 | 20 | 24, 95 | 100 | 103, 176 | 180 | 184).  Asserted: ten times the measured gap,
    and the measured slack, which is testers.QUANTILE_COUNT_SLACK."""
    D, s, runs = quantile_runs
    r = runs[tau]
    fun, _ = _quantile_lp(D, s, tau, 1.0 - tau)
    gap = (float(r["objopt"]) - fun) / fun
    z = np.asarray(r["zopt"]).reshape(-1)
    slack = ap.testers.quantile_count_slack(z, tau)
    print(f"tau = {tau}: LP {fun:.9f}, objopt {float(r['objopt']):.9f}, gap {gap:+.3e}, {int(r['steps'])} steps; "
          f"#(z<0) = {np.sum(z < 0)}, #(z==0) = {np.sum(z == 0)}, tau*m = {tau * z.size:g}, slack {slack:g}")
    assert abs(gap) <= 10 * MEASURED_GAP
    assert slack <= ap.testers.QUANTILE_COUNT_SLACK == 0


def test_quantile_fits_bracket_lad(quantile_runs):
    """tau = 0.1 and 0.9 differ from LAD (tau = 0.5 up to the factor 1/2) and bracket it: with phi_tau on z = D*x - s a
    fraction tau of the residuals is negative, so the fit rises with 1 - tau -- the intercept and the mean fitted value"""
    D, _, runs = quantile_runs
    x = {tau: np.asarray(r["xopt"]).reshape(-1) for tau, r in runs.items()}
    fit = {tau: float(np.mean(D @ x[tau])) for tau in x}
    print("intercepts", {t: x[t][0] for t in x}, "mean fits", fit)
    assert np.linalg.norm(x[0.1] - x[0.5]) > 0.1 and np.linalg.norm(x[0.9] - x[0.5]) > 0.1
    assert x[0.9][0] < x[0.5][0] < x[0.1][0]
    assert fit[0.9] < fit[0.5] < fit[0.1]


# ------------------------------------------------------------------------------------ (e) binding layer (no device)
def _binding(ap, kind="lad", **extra):
    from admm_project_amd.binding import Binding
    rng = np.random.default_rng(3)
    args = dict(D=rng.standard_normal((12, 8)), s=rng.standard_normal(12))
    args.update(extra)
    return Binding(kind, args)


@pytest.mark.parametrize("kind,extra", [
    ("lad", dict(weights=np.ones(11))),
    ("huberfit", dict(weights=np.ones(11))),
    ("lad", dict(weights=np.ones(13))),
    ("lad", dict(weights=[1.0] * 11 + [-1.0])),
    ("lad", dict(weights=[1.0] * 11 + [float("nan")])),
    ("lad", dict(tau=0.0)),
    ("lad", dict(tau=1.0)),
    ("lad", dict(tau=1.5)),
    ("lad", dict(tau=float("nan"))),
    ("lad", dict(tau=0.3, slopes=[0.3, 0.7])),
    ("lad", dict(slopes=[0.3, 0.0])),
    ("lad", dict(slopes=[0.3, 0.3, 0.4])),
    ("huberfit", dict(epsilon=0.1)),
    ("lad", dict(epsilon=-0.1)),
    ("lad", dict(delta=0.5)),
    ("huberfit", dict(delta=0.0)),
], ids=["short", "short-huber", "long", "negative", "nan", "tau=0", "tau=1", "tau>1", "tau-nan", "tau+slopes", "slope=0",
        "three-slopes", "eps-on-huber", "eps<0", "delta-on-lad", "delta=0"])
def test_binding_refuses(ap, kind, extra):
    with pytest.raises(ap.AdmmError) as ei:
        _binding(ap, kind, **extra)
    assert ei.value.code == ap._lib.E_INVALID, str(ei.value)


def test_binding_accepts_the_family(ap):
    for kind, extra in (("lad", dict(weights=np.linspace(0.0, 2.0, 12))), ("lad", dict(tau=0.9)),
                        ("lad", dict(slopes=[0.2, 0.8], epsilon=0.3)), ("lad", dict(delta=1.0)),
                        ("huberfit", dict(weights=np.ones(12), slopes=[1.5, 0.5], delta=0.5)), ("huberfit", dict(epsilon=0.0))):
        b = _binding(ap, kind, **extra)
        assert b.info()["problem"] == (ap._lib.PROB_LAD if kind == "lad" else ap._lib.PROB_HUBERFIT)
        assert b.info()["nA"] == 8 and b.info()["nB"] == 12
        b.close()


# ------------------------------------------------------------------------------------ Python surfaces
@pytest.mark.parametrize("opts", [
    dict(weights=np.ones(11)), dict(weights=[1.0] * 11 + [-1.0]), dict(tau=0.0), dict(tau=1.0),
    dict(tau=0.3, slopes=(0.3, 0.7)), dict(slopes=(1.0, -1.0)), dict(epsilon=-1.0), dict(delta=0.5),
], ids=["short", "negative", "tau=0", "tau=1", "tau+slopes", "slope<0", "eps<0", "delta-on-lad"])
def test_lad_raises_in_python(ap, monkeypatch, opts):
    """before getproxops is reached: nothing here may touch the library"""
    import admm_project_amd.solvers as S
    monkeypatch.setattr(S, "getproxops", lambda *a, **k: pytest.fail("getproxops was reached"))
    rng = np.random.default_rng(4)
    D, s = rng.standard_normal((12, 8)), rng.standard_normal(12)
    with pytest.raises(ValueError):
        ap.lad(D, s, opts)
    with pytest.raises(ValueError):
        ap.huberfit(D, s, dict(epsilon=0.2))
    with pytest.raises(ValueError):
        ap.quantilereg(D, s, 1.0, {})
    with pytest.raises(ValueError):
        ap.quantilereg(D, s, 0.5, dict(slopes=(1.0, 1.0)))
    with pytest.raises(TypeError):
        ap.quantilereg(D, s, 0.5, None)


def test_getproxops_checks_the_family_before_the_engine(ap, monkeypatch):
    import admm_project_amd.api as A
    monkeypatch.setattr(A, "Engine", lambda *a, **k: pytest.fail("an engine was created"))
    with pytest.raises(ValueError):
        ap.getproxops("LAD", dict(D=np.zeros((12, 8)), s=np.zeros(12), weights=np.ones(11)))
    with pytest.raises(ValueError):
        ap.getproxops("HuberFit", dict(D=np.zeros((12, 8)), s=np.zeros(12), epsilon=0.5))


def test_abi_is_unchanged_and_the_symbols_are_exported(ap):
    import ctypes as C
    L = ap._lib
    assert L.load().admm_abi_version() == L.ABI_VERSION == 5
    assert C.sizeof(L.EngineInfo) == 120 and C.sizeof(L.LossDesc) == 40
    for name in ("admm_engine_set_loss", "admm_engine_get_loss", "admm_op_loss_prox"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(L.load(), name)
    assert "quantilereg" in ap.solvers.__all__ and "quantileregtest" in ap.testers.__all__
    assert hasattr(ap.Engine, "set_loss") and hasattr(ap, "quantilereg")
