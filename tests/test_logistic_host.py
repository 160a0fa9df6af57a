"""lossfunction = 'logistic' without a device: the NumPy restatement (tests/logistic_restated.py) against long double
and against a Newton minimiser of the problem it claims to solve, and the string -> ADMM_LOSS_* mapping of the binding
layer and the Python surfaces."""
import numpy as np
import pytest

import logistic_restated as R


def test_restated_prox_against_long_double():
    """the yardstick of the device test (test_gpu_logistic): max |s - s_ld| / (eps*(|w| + t + 1)) of the fp64
    restatement over the grid and 4000 random pairs.  Measured: 0.986"""
    assert np.finfo(np.longdouble).eps < 1e-18  # (an 80-bit long double: the exact value means something)
    gw, gt = R.grid_pairs()
    rw, rt = R.random_pairs()
    w, t = np.concatenate([gw, rw]), np.concatenate([gt, rt])
    s64 = R.prox_root(w, t)
    sld = R.prox_root(w, t, np.longdouble)
    assert np.isfinite(s64).all() and np.isfinite(np.asarray(sld, dtype=np.float64)).all()
    assert np.all(s64 >= w) and np.all(s64 <= w + t)
    r = R.ratio(s64, sld, w, t)
    print(f"restated prox: max |s - s_ld| / (eps*(|w| + t + 1)) = {r.max():.3f} at w = {w[r.argmax()]!r}, "
          f"t = {t[r.argmax()]!r}")
    assert r.max() <= 2.0
    zero = t == 0.0
    assert np.array_equal(s64[zero], w[zero])  # t = 0: the argument itself
    # the long-double roots are roots: |phi| at rounding level of the terms
    one = np.longdouble(1)
    with np.errstate(over="ignore"):
        phi = (sld - w) - t / (one + np.exp(sld))
    assert np.all(np.abs(phi) <= 4 * np.finfo(np.longdouble).eps * (np.abs(w) + t + 1))


def test_restated_run_solves_the_logistic_problem(ap):
    """256 x 2 (not separable), forced through all 1000 iterations: xopt against a Newton minimiser of
    sum log(1 + exp(-ell.*(D*x))), whose minimiser does not depend on C.  The two bands nearly separate, the minimiser
    is long (|x| = 15.8) and ADMM at rho = 1 approaches it slowly: the relative distance falls 0.869, 0.618, 0.381, 0.266
    after 10, 100, 500, 1000 iterations.  Measured distance of xopt: 0.26615740098067703 (the pin is twice that)"""
    p = ap.synth.svm_problem(0)
    D, ell = p["D"], p["ell"]
    res = R.run(D, ell, p["C"], dict(domaxiters=1, x0=p["x0"], z0=p["z0"], u0=p["u0"]))
    assert res["steps"] == 1000
    A = ell[:, None] * D
    x = np.zeros(D.shape[1])
    for _ in range(60):  # Newton on the smooth, strictly convex sum (D has full column rank)
        q = A @ x
        sg = np.exp(-np.logaddexp(0.0, q))  # 1/(1 + e^q)
        grad = -A.T @ sg
        H = A.T @ ((sg * (1 - sg))[:, None] * A)
        x = x - np.linalg.solve(H, grad)
    assert np.linalg.norm(A.T @ np.exp(-np.logaddexp(0.0, A @ x))) < 1e-12
    dist = float(np.linalg.norm(res["xopt"] - x) / np.linalg.norm(x))
    print(f"restated run after 1000 iterations: |xopt - x_newton| / |x_newton| = {dist:.3e}")
    assert dist <= 2 * MEASURED_DISTANCE
    d = [float(np.linalg.norm(res["xvals"][:, i] - x)) for i in (9, 99, 499, 999)]
    assert d[0] > d[1] > d[2] > d[3]  # and it is on its way there
    assert R.loss_sum(A @ x) < R.loss_sum(A @ res["xopt"]) < R.loss_sum(A @ res["xvals"][:, 99])


MEASURED_DISTANCE = 0.26615740098067703


@pytest.mark.parametrize("text,code", [("logistic", 3), ("Logistic", 3), ("hinge", 0), ("Hinge", 0), ("01", 1),
                                       ("hinge01", 2), ("0-1", 2), (None, 0)])
def test_binding_maps_the_loss_strings(ap, text, code):
    from admm_project_amd import binding as B
    args = dict(D=np.eye(4, 2), Dt=np.eye(2, 4), ell=np.ones(4), C=0.5)
    if text is not None:
        args["lossfunction"] = text
    b = B.Binding("LinearSVM", args)
    try:
        assert b.desc.loss == code
    finally:
        b.close()


def test_python_surfaces_map_the_loss_strings(ap):
    L = ap._lib
    assert L.LOSS_LOGISTIC == 3
    assert [L.loss_code(s) for s in ("logistic", "Logistic", "hinge", "01", "hinge01", "0-1", "Hinge")] == \
        [3, 3, 0, 1, 2, 2, 2]  # ('Hinge' through getproxops in Python was, and stays, case-sensitive)


def test_ovr_argument_checks_accept_a_mixed_list(ap):
    """the host-side checks of linearsvm_ovr pass a mixed loss list on to the engine (which needs a device) and still
    refuse a list of the wrong length"""
    rng = np.random.default_rng(0)
    D = rng.random((40, 3))
    labels = rng.integers(0, 3, size=40).astype(np.float64)
    with pytest.raises(ValueError):
        ap.linearsvm_ovr(D, labels, 0.5, dict(lossfunction=["logistic", "hinge"]))
    try:
        got = ap.linearsvm_ovr(D, labels, 0.5, dict(lossfunction=["logistic", "hinge", "01"]))
    except ap._lib.AdmmError as e:  # no device here: the checks were passed, the engine was reached
        assert ap._lib.device_count() <= 0 and "no HIP device" in str(e)
    else:
        assert got["xopt"].shape == (3, 3) and np.isfinite(got["xopt"]).all()
