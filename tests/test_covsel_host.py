"""Covariance selection, host side: the restated reference closures, the tester's problem recipe and the refusals that
must come before any device work (no GPU needed)."""
import numpy as np
import pytest

from covsel_restated import cov, oracle_run, samples, xprox


def test_xprox_solves_the_optimality_condition():
    # getProxOps.m:1487-1495 minimises trace(S X) - log det X + rho/2 ||X - (Z - U)||_F^2:  rho*X - inv(X) = rho*(Z - U) - S
    rng = np.random.default_rng(3)
    n = 24
    S = cov(samples(1, 200, n))
    for rho in (0.1, 1.0, 10.0):
        Z = rng.standard_normal((n, n))
        Z = Z + Z.T
        U = rng.standard_normal((n, n))
        U = U + U.T
        X = xprox(S, Z, U, rho)
        lhs = rho * X - np.linalg.inv(X)
        rhs = rho * (Z - U) - S
        assert np.linalg.norm(lhs - rhs) <= 1e-12 * max(1.0, np.linalg.norm(rhs))
        assert np.min(np.linalg.eigvalsh(0.5 * (X + X.T))) > 0.0


def test_oracle_tends_to_the_inverse_as_lambda_vanishes():
    n = 8
    S = cov(samples(2, 400, n))
    res = oracle_run(S, 1e-10, dict(rho=1.0, maxiters=2000, abstol=1e-10, reltol=1e-10))
    X = res["xopt"].reshape((n, n), order="F")
    Sinv = np.linalg.inv(S)
    assert np.linalg.norm(X - Sinv) <= 1e-6 * np.linalg.norm(Sinv)


def test_synth_problem_is_spd_and_reproducible(ap):
    a = ap.synth.covsel_problem(seed=4)
    b = ap.synth.covsel_problem(seed=4)
    c = ap.synth.covsel_problem(seed=5)
    Sinv = a["Sinv"]
    assert a["D"].shape == (2 ** 9, 2 ** 6)
    assert np.array_equal(Sinv, Sinv.T)
    assert np.min(np.linalg.eigvalsh(Sinv)) > 0.0
    assert np.all(np.diag(Sinv) >= 2.0)  # I + I', plus the shift when the sprinkle made it indefinite
    for k in ("D", "S", "Sinv"):
        assert np.array_equal(a[k], b[k])
    assert not np.array_equal(a["D"], c["D"])
    assert np.allclose(a["S"] @ Sinv, np.eye(Sinv.shape[0]), atol=1e-12)


def test_host_refusals_come_before_the_device(ap, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work started")

    monkeypatch.setattr(ap.api, "Engine", no_device)
    with pytest.raises(KeyError, match="args.S"):
        ap.getproxops("covarianceselection", {"lambda": 1.0})
    with pytest.raises(KeyError, match="args.lambda"):
        ap.getproxops("covarianceselection", {"S": np.eye(3)})
    with pytest.raises(ValueError, match="square"):
        ap.getproxops("covarianceselection", {"S": np.ones((3, 4)), "lambda": 1.0})
    with pytest.raises(ValueError, match="square"):
        ap.getproxops("covarianceselection", {"S": np.ones(3), "lambda": 1.0})
    D = samples(0, 16, 4)
    with pytest.raises(ValueError, match="positive real"):
        ap.covarianceselection(D, 0.0)
    with pytest.raises(ValueError, match="positive real"):
        ap.covarianceselection(D, -1.0)
    with pytest.raises(ValueError, match="not a matrix"):
        ap.covarianceselection(D[:, 0], 1.0)
    with pytest.raises(TypeError, match="struct"):
        ap.covarianceselection(D, 1.0, options=[])


def test_public_surface(ap):
    assert callable(ap.covarianceselection)
    assert "covarianceselection" in ap.solvers.__all__
    assert "covarianceselectiontest" in ap.testers.__all__
    assert ap._lib.PROB_COVSEL == 13
