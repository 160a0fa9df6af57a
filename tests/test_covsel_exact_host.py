"""The exact covariance-selection reference (tests/covsel_exact.py) on the host: the constructions are exact, mpmath's
f matches both closed forms where they do not cancel, and the error bound accepts numpy's stable-form result while it
rejects each plausible eigen-step bug, simulated at n = 64 (the one-workgroup path) and n = 300 (the one-sided path)."""
import math

import mpmath
import numpy as np
import pytest

import covsel_exact as ce


@pytest.mark.parametrize("n", [1, 2, 5, 64, 95, 96, 97, 129, 256, 300, 1024])
def test_construction_is_exact(n):
    s = ce.spectrum("quarter-repeated", n, n)
    E = ce.Exact(s, n + 1)
    assert sum(E.sizes) == n
    assert np.array_equal(E.Q.T @ E.Q, np.eye(n))
    assert np.array_equal(E.S, E.S.T)
    assert np.array_equal(E.Q.T @ E.S @ E.Q, np.diag(s))
    assert set(np.unique(np.abs(E.Q[E.Q != 0]))) <= {2.0 ** -k for k in range(6)}


@pytest.mark.parametrize("kind", ["equal", "half-repeated", "zeros", "range", "mixed", "cluster"])
def test_exact_x_is_the_matrix_function(kind):
    n, rho = 97, 1.0
    s = ce.spectrum(kind, n, 3)
    E = ce.Exact(s, 4)
    X, nld, trSX, fm = E.X(-s, rho)
    assert np.array_equal(X, X.T)
    # Q' X Q = diag(f) up to the one rounding of each entry of X
    fd = np.array([float(v) for v in fm])
    R = E.Q.T @ X @ E.Q
    assert np.max(np.abs(R - np.diag(fd))) <= 4 * n * ce.EPS * np.max(np.abs(X))
    # numpy's stable-form X is within the bound; so are -log det and trace(S X)
    Xr, lam = ce.x_ref(-E.S, rho)
    assert np.linalg.norm(Xr - X) <= ce.x_bound(lam, np.linalg.norm(E.S), np.linalg.norm(X), rho, n)
    assert abs(-np.sum(np.log(ce.f_stable(lam, rho))) - float(nld)) <= ce.logdet_bound(lam, np.linalg.norm(E.S), rho, n)
    assert abs(float(trSX) - np.sum(E.S * X)) <= 1e-12 * max(1.0, np.sum(np.abs(E.S * X)))


def test_exact_logdet_where_det_overflows_and_underflows():
    n = 256
    E = ce.Exact(ce.spectrum("all-zero", n, 0), 1)
    for rho, sign in ((2.0 ** -20, 1), (2.0 ** 20, -1)):  # f(0) = 1/sqrt(rho) = 2^(+-10): det = 2^(+-2560)
        X, nld, _, _ = E.X(np.zeros(n), rho)
        assert np.array_equal(X, np.eye(n) * 2.0 ** (sign * 10))
        assert float(nld) == pytest.approx(-sign * 10 * n * math.log(2.0), rel=1e-15)
        with np.errstate(over="ignore", under="ignore"):
            assert not (0.0 < np.linalg.det(X) < np.inf)  # the literal log(det(x)) is not an option here
        assert np.linalg.slogdet(X)[1] == pytest.approx(-float(nld), rel=1e-14)


@pytest.mark.parametrize("rho", [2.0 ** -20, 1.0, 2.0 ** 20])
def test_mp_f_matches_both_closed_forms(rho):
    lam = np.concatenate([-np.logspace(-6, 6, 25) * math.sqrt(rho), [0.0], np.logspace(-6, 6, 25) * math.sqrt(rho)])
    ref = np.array([float(ce.f_mp(l, rho)) for l in lam])
    np.testing.assert_allclose(ce.f_stable(lam, rho), ref, rtol=4 * ce.EPS, atol=0)
    ok = lam >= -math.sqrt(rho)  # no cancellation in the literal form
    np.testing.assert_allclose(ce.f_literal(lam[ok], rho), ref[ok], rtol=8 * ce.EPS, atol=0)
    # and the literal form does cancel far left: the reason the kernel (and this reference) use the stable one
    assert np.max(np.abs(ce.f_literal(lam[~ok], rho) / ref[~ok] - 1.0)) > 1e-6
    # f' is f / sqrt(l^2 + 4 rho)
    with mpmath.workdps(ce.DPS):
        for l in lam[::7]:
            d = mpmath.diff(lambda t: (t + mpmath.sqrt(t * t + 4 * rho)) / (2 * rho), mpmath.mpf(float(l)))
            assert float(ce.fprime(l, rho)) == pytest.approx(float(d), rel=1e-12)


def test_cov_reference_and_bound():
    rng = np.random.default_rng(0)
    D = rng.standard_normal((1001, 30)) + 1e8
    S, A = ce.cov_ref(D)
    B = ce.cov_bound(D, A)
    assert np.all(np.abs(np.asarray(S, dtype=np.float64) - np.cov(D, rowvar=False)) <= B)
    # the one-pass D'D - m mu mu' cancels: far outside the bound
    m = D.shape[0]
    mu = D.mean(axis=0)
    one_pass = (D.T @ D - m * np.outer(mu, mu)) / (m - 1)
    assert np.any(np.abs(one_pass - np.asarray(S, dtype=np.float64)) > 100 * B)


# ---------------------------------------------------------------------------------------------------- teeth
def jacobi_two_sided(M, V0, sweeps=None, tol=ce.EPS):
    """The small path's algorithm on the host: A = V0' M V0, then cyclic two-sided Jacobi in the round-robin parallel
    order until a sweep rotates nothing (or after `sweeps` sweeps).  Returns (diag A, V, sweeps done)."""
    n = M.shape[0]
    A = V0.T @ M @ V0
    A = np.tril(A) + np.tril(A, -1).T
    V = V0.copy()
    ne = n + (n & 1)
    absfloor = 1e-3 * ce.EPS * np.linalg.norm(M)
    done = 0
    for sweep in range(sweeps if sweeps is not None else 40):
        rot = 0
        for r in range(ne - 1):
            # round-robin tournament: player ne-1 fixed, the others rotate
            idx = [(r + k) % (ne - 1) for k in range(ne - 1)] + [ne - 1]
            p = np.array([idx[k] for k in range(ne // 2)])
            q = np.array([idx[ne - 1 - k] for k in range(ne // 2)])
            keep = q < n
            p, q = np.minimum(p[keep], q[keep]), np.maximum(p[keep], q[keep])
            keep = p < n
            p, q = p[keep], q[keep]
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            act = (np.abs(apq) > absfloor) & (np.abs(apq) > tol * np.sqrt(np.abs(app * aqq)))
            if not np.any(act):
                continue
            p, q, app, aqq, apq = p[act], q[act], app[act], aqq[act], apq[act]
            rot += p.size
            theta = (aqq - app) / (2.0 * apq)
            t = np.sign(theta + (theta == 0)) / (np.abs(theta) + np.sqrt(1.0 + theta * theta))
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = t * c
            Ap, Aq = A[:, p].copy(), A[:, q].copy()
            A[:, p], A[:, q] = c * Ap - s * Aq, s * Ap + c * Aq
            Vp, Vq = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = c * Vp - s * Vq, s * Vp + c * Vq
            Ap, Aq = A[p, :].copy(), A[q, :].copy()
            A[p, :], A[q, :] = c[:, None] * Ap - s[:, None] * Aq, s[:, None] * Ap + c[:, None] * Aq
            A[p, q] = A[q, p] = 0.0
        done += 1
        if rot == 0:
            break
    return np.diag(A).copy(), V, done


def _case(n, seed=0):
    """A dense M with a wide spread of f' (both signs, |l| up to ~10 sqrt(rho)) and its exact X."""
    s = ce.spectrum("mixed", n, seed) * 4.0
    E = ce.Exact(s, seed + 1)
    rho = 1.0
    X, nld, _, _ = E.X(-s, rho)
    M = -E.S
    lam = np.sort(-s)
    return E, M, X, lam, rho


def _rejected(Xbad, X, M, lam, rho):
    n = M.shape[0]
    b = ce.x_bound(lam, np.linalg.norm(M), np.linalg.norm(X), rho, n)
    r = ce.ratio(np.linalg.norm(Xbad - X), b)
    assert r > 1.0, r
    return r


@pytest.mark.parametrize("n", [64, 300])
def test_bound_accepts_numpy(n):
    E, M, X, lam, rho = _case(n)
    Xr, lr = ce.x_ref(M, rho)
    assert np.linalg.norm(Xr - X) <= 0.1 * ce.x_bound(lr, np.linalg.norm(M), np.linalg.norm(Xr), rho, n)
    # the host model of the kernel's two-sided Jacobi passes too, from I and from a nearby basis
    for V0 in (np.eye(n), np.linalg.eigh(M + 1e-3 * np.diag(np.linspace(-1, 1, n)))[1]):
        d, V, _ = jacobi_two_sided(M, V0)
        Xj = (V * ce.f_stable(d, rho)) @ V.T
        assert np.linalg.norm(Xj - X) <= ce.x_bound(lr, np.linalg.norm(M), np.linalg.norm(X), rho, n)


@pytest.mark.parametrize("n", [64, 300])
def test_bound_rejects_the_literal_f(n):
    s = ce.spectrum("positive-large", n, 5)  # M = -S: eigenvalues in [-2^20, -2^16], rho = 1: l << -sqrt(rho)
    E = ce.Exact(s, 6)
    rho = 1.0
    X, _, _, _ = E.X(-s, rho)
    lam, V = np.linalg.eigh(-E.S)
    _rejected((V * ce.f_literal(lam, rho)) @ V.T, X, -E.S, lam, rho)
    assert np.linalg.norm((V * ce.f_stable(lam, rho)) @ V.T - X) <= ce.x_bound(lam, np.linalg.norm(E.S),
                                                                                 np.linalg.norm(X), rho, n)


@pytest.mark.parametrize("n", [64, 300])
def test_bound_rejects_a_basis_off_orthogonal(n):
    E, M, X, lam, rho = _case(n)
    l, V = np.linalg.eigh(M)
    rng = np.random.default_rng(1)
    G = rng.standard_normal((n, n))
    G = 0.5 * (G + G.T)
    Vb = V @ (np.eye(n) + 1e-10 * G / np.linalg.norm(G, 2))  # ||V'V - I||_2 ~ 2e-10
    _rejected((Vb * ce.f_stable(l, rho)) @ Vb.T, X, M, lam, rho)


@pytest.mark.parametrize("n", [64, 300])
def test_bound_rejects_jacobi_one_sweep_short(n):
    E, M, X, lam, rho = _case(n)
    rng = np.random.default_rng(2)
    P = rng.standard_normal((n, n))
    V0 = np.linalg.eigh(M + 1e-2 * (P + P.T) / math.sqrt(n))[1]  # the previous x-update's basis: V0' M V0 nearly diagonal
    b = ce.x_bound(lam, np.linalg.norm(M), np.linalg.norm(X), rho, n)
    Xk = []  # X after k sweeps, k = 0 .. the converged count (whose last sweep rotates nothing: the stop test)
    k = 0
    while True:
        d, V, done = jacobi_two_sided(M, V0, sweeps=k)
        Xk.append((V * ce.f_stable(d, rho)) @ V.T)
        if done < k:  # converged after `done` sweeps
            break
        k += 1
    sweeps = len(Xk) - 2
    assert np.linalg.norm(Xk[-1] - X) <= b
    # under quadratic convergence the sweeps before the stop test may only polish rounding: the last sweep that
    # converges is the last one that moves X by more than the allowance for rounding (the bound); stop just before it
    last = max(k for k in range(1, sweeps + 1) if np.linalg.norm(Xk[k] - Xk[k - 1]) > b)
    assert last >= 2
    _rejected(Xk[last - 1], X, M, lam, rho)


@pytest.mark.parametrize("n", [64, 300])
def test_bound_rejects_a_shifted_spectrum(n):
    E, M, X, lam, rho = _case(n)
    # the large path's shift: sigma = max(0, -min Gershgorin lower end) + 1e-3 max Gershgorin upper end
    rad = np.sum(np.abs(M), axis=0) - np.abs(np.diag(M))
    sigma = max(0.0, -np.min(np.diag(M) - rad)) + 1e-3 * np.max(np.abs(np.diag(M)) + rad)
    l, V = np.linalg.eigh(M)
    _rejected((V * ce.f_stable(l + 1e3 * ce.EPS * sigma, rho)) @ V.T, X, M, lam, rho)


@pytest.mark.parametrize("n", [64, 300])
def test_bound_rejects_the_upper_triangle(n):
    E, M, X, lam, rho = _case(n)
    S = E.S
    # an S the engine accepts (|S - S'| <= 1e-12 max|S|), with the whole tolerance used above the diagonal
    rng = np.random.default_rng(3)
    Su = S + np.triu(rng.choice([-1.0, 1.0], (n, n)), 1) * 1e-12 * np.max(np.abs(S)) * (1 - 1e-3)
    assert np.max(np.abs(Su - Su.T)) <= 1e-12 * np.max(np.abs(Su))
    Xl, _ = ce.x_ref(-Su, rho)  # UPLO = 'L': the engine's semantics, within the bound
    assert np.linalg.norm(Xl - X) <= ce.x_bound(lam, np.linalg.norm(M), np.linalg.norm(X), rho, n)
    lu, Vu = np.linalg.eigh(-Su, UPLO="U")
    Xu = (Vu * ce.f_stable(lu, rho)) @ Vu.T
    _rejected(Xu, X, M, lam, rho)
