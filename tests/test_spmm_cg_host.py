"""The lock-step CG of the sparse multi-fit solvers without a device: the float64 restatement against the
longdouble one over every case of test_gpu_spmm_cg (this MEASURES the two bounds of that file), the guard that lets an
iteration count be compared at all, the longdouble restatement against an exact rational solve, and the refusals of
admm_op_spmm_cg that fire before the device is touched."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import spmm_cg_restated as R
from sparse_cases import Csc, csc_of, desc_of

LD = np.longdouble


def test_float64_against_longdouble_measures_the_bounds(ap):
    """per fit of every case: the gap in x at equal iteration count relative to ||x||_inf, and the distance between the
    norm of the recurrence's residual and the norm of the true one, and the norm of their difference, relative to ||y||; the
    recorded constants cover all three"""
    worst_gap, worst_drift, worst_vec = (0.0, None), (0.0, None), (0.0, None)
    for name, case in R.CASES.items():
        c = R.inputs(ap, name)
        f64 = R.restated(ap, name, np.float64)
        ld = R.reference(ap, name)
        for k, (a, b) in enumerate(zip(f64, ld)):
            assert [a[f] for f in ("iters", "brk", "zero")] == [b[f] for f in ("iters", "brk", "zero")], (name, k)
            xinf = float(np.max(np.abs(b["x"])))
            if xinf == 0.0:
                assert not a["x"].any(), (name, k)
            else:
                gap = float(np.max(np.abs(a["x"].astype(LD) - b["x"]))) / xinf
                worst_gap = max(worst_gap, (gap, f"{name}, fit {k}, {a['iters']} iterations"))
            ynorm = float(np.linalg.norm(c["Y"][:, k]))
            if ynorm > 0.0:
                rt = R.true_residual(c["A"], c["Y"][:, k], a["x"], case.shift)
                rnorm = np.linalg.norm(a["r"].astype(LD))
                drift = float(abs(rnorm - np.linalg.norm(rt))) / ynorm
                vec = float(np.linalg.norm(a["r"].astype(LD) - rt)) / ynorm
                worst_drift = max(worst_drift, (drift, f"{name}, fit {k}, {a['iters']} iterations"))
                worst_vec = max(worst_vec, (vec, f"{name}, fit {k}, {a['iters']} iterations"))
    print(f"MEASURED_X_GAP: {worst_gap[0]:.3e} ({worst_gap[1]}); recorded {R.MEASURED_X_GAP:g}")
    print(f"MEASURED_DRIFT: {worst_drift[0]:.3e} ({worst_drift[1]}); recorded {R.MEASURED_DRIFT:g}")
    print(f"MEASURED_R_GAP: {worst_vec[0]:.3e} ({worst_vec[1]}); recorded {R.MEASURED_R_GAP:g}")
    assert worst_gap[0] <= R.MEASURED_X_GAP
    assert worst_drift[0] <= R.MEASURED_DRIFT
    assert worst_vec[0] <= R.MEASURED_R_GAP


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c.counts])
def test_no_compared_iteration_count_can_flip(ap, name):
    """sqrt(rs) / (tol*||y||) of the float64 restatement lies outside [0.5, 2] at the last inner iteration and at the one
    before it, for every fit whose count test_gpu_spmm_cg compares; and the longdouble restatement, left to its own stop
    test, ends with the same counters: the count is a property of the operation, not of its rounding"""
    for k, (res, ld) in enumerate(zip(R.restated(ap, name, np.float64), R.restated(ap, name, LD))):
        tail = ", ".join(f"{v:.3g}" for v in res["ratios"][-2:])
        print(f"{name}, fit {k}: {res['iters']} iterations, capped {res['capped']}, brk {res['brk']}, zero {res['zero']}, "
              f"last ratios [{tail}]; longdouble: {ld['iters']} iterations")
        assert R.guard(res), (name, k, res["ratios"][-2:])
        assert R.stable(res, ld), (name, k, ld["iters"], ld["ratios"][-2:])


def test_the_cases_reach_what_they_are_for(ap):
    its = lambda name: [r["iters"] for r in R.restated(ap, name, np.float64)]
    assert its("mixed")[0] == 1 and min(its("mixed")[1:]) > 20
    assert min(its("A65 shift 2.5")) > 9  # the matrix and shift of the cap, unbounded
    for maxit in (1, 3, 5, 9):
        assert all(r["iters"] == maxit and r["capped"] == 1 for r in R.restated(ap, f"maxit {maxit}", np.float64))
    for name in ("brk", "brk warm"):
        r = R.restated(ap, name, np.float64)[1]
        assert (r["iters"], r["capped"], r["brk"]) == (1, 1, 1)
    assert not R.restated(ap, "brk", np.float64)[1]["x"].any()
    assert np.array_equal(R.restated(ap, "brk warm", np.float64)[1]["x"], R.inputs(ap, "brk warm")["X0"][:, 1])
    r = R.restated(ap, "e7 shift 2", np.float64)[1]
    assert (r["iters"], r["capped"], r["brk"], r["x"][R.EMPTY_COLUMN], np.count_nonzero(r["x"])) == (1, 0, 0, 0.5, 1)
    for name in ("zero", "zero warm"):
        r = R.restated(ap, name, np.float64)[1]
        assert (r["iters"], r["capped"], r["zero"]) == (0, 0, 1) and not r["x"].any()
    assert R.inputs(ap, "zero warm")["X0"][:, 1].any()
    assert all(r["iters"] == 0 and r["capped"] == 0 for r in R.restated(ap, "converged", np.float64))
    assert len({r["iters"] for r in R.restated(ap, "WIDE shift 0", np.float64)} | {0}) > 1
    assert R.matrix(ap, R.WIDE).shape[1] > 32 * 256
    for n, shape in R.TINY.items():
        assert R.matrix(ap, shape).shape[1] == n
    Y = R.inputs(ap, "A65 shift 2.5")["Y"]  # six orders of magnitude across the columns
    norms = np.linalg.norm(Y, axis=0)
    assert norms[-1] / norms[0] > 1e5


# ---- the reference against an exact solve
def _integers(M):
    """(object array of Python ints, L): M * L exactly, L the largest denominator (every float64 is dyadic)"""
    F = [[Fraction(float(v)) for v in row] for row in np.atleast_2d(M)]
    L = max(max(v.denominator for v in row) for row in F)
    return np.array([[int(v * L) for v in row] for row in F], dtype=object).reshape(np.shape(M)), L


def _exact_solve(A, shift, Y):
    """(D'D + shift*I)^-1 Y in rational arithmetic, as (integer numerators, one integer denominator): fraction-free (Bareiss) elimination and substitution on
    integers, on the n x n matrix itself or, for a fat D, on the m x m one of x = (y - D'(DD' + shift*I)^-1 D y) / shift"""
    m, n = A.shape
    shift = Fraction(shift)
    Ai, L = _integers(A)
    L *= shift.denominator
    Ai = Ai * shift.denominator
    Yi, Ly = _integers(Y)
    small = m < n
    N = min(m, n)
    # L^2 (G + shift*I) W = L^2 B with W' = Ly*W: integers on both sides
    G = (Ai @ Ai.T if small else Ai.T @ Ai) + int(shift * L * L) * np.eye(N, dtype=object)
    B = L * (Ai @ Yi) if small else L * L * Yi
    M = np.concatenate([G, B], axis=1)
    prev = 1
    for k in range(N - 1):  # (symmetric positive definite: every pivot is a leading minor > 0)
        M[k + 1:, k + 1:] = (M[k + 1:, k + 1:] * M[k, k] - np.outer(M[k + 1:, k], M[k, k + 1:])) // prev
        M[k + 1:, k] = 0
        prev = M[k, k]
    det = M[N - 1][N - 1]
    W = np.empty((N, Y.shape[1]), dtype=object)  # det * W', integers by Cramer's rule: every division below is exact
    for c in range(Y.shape[1]):
        for i in range(N - 1, -1, -1):
            num = M[i][N + c] * det - sum(M[i][j] * W[j, c] for j in range(i + 1, N))
            assert num % M[i][i] == 0
            W[i, c] = num // M[i][i]
    if not small:
        return W, det * Ly
    X = L * det * Yi - Ai.T @ W  # x = (y - D'W) / shift
    return X * shift.denominator, det * Ly * L * shift.numerator


def _fraction_of(v):
    """a longdouble exactly"""
    hi = float(v)
    return Fraction(hi) + Fraction(float(v - LD(hi)))


@pytest.mark.parametrize("name,cols", [("A65 shift 1", (0, 10)), ("FAT shift 2.5", (0, 9))])
def test_longdouble_restatement_against_an_exact_solve(ap, name, cols):
    """||x - x_exact|| / ||x_exact|| <= cond * 1e-15 at tol = 1e-15: the error of a solution whose residual is r is at
    most cond * ||r|| / ||y|| relative, in the 2-norm"""
    c = R.inputs(ap, name)
    A, shift = c["A"], c["case"].shift
    Y = c["Y"][:, list(cols)]
    ev = np.linalg.eigvalsh(A.T @ A) + shift
    cond = float(ev.max() / ev.min())
    num, den = _exact_solve(A, shift, Y)
    for j, k in enumerate(cols):
        res = R.cg(A, Y[:, j], None, shift, 1e-15, 1000, LD)
        assert res["capped"] == 0
        err2 = ref2 = 0.0
        for v, e in zip(res["x"], num[:, j]):  # (x - e/den = (p*den - e*q) / (q*den) for x = p/q: exact, then one rounding)
            f = _fraction_of(v)
            err2 += ((f.numerator * den - int(e) * f.denominator) / (f.denominator * den)) ** 2
            ref2 += (int(e) / den) ** 2
        rel = float(np.sqrt(err2 / ref2))
        print(f"{name}, fit {k}: {res['iters']} iterations, cond {cond:.3g}, relative error {rel:.3e} "
              f"(bound {cond * 1e-15:.3e})")
        assert rel <= cond * 1e-15


# ---- the operator's refusals
def _valid(ap):
    c = R.inputs(ap, "A65 shift 1")
    return c["D"], c["Y"][:, :3]


def refusal_cases(ap):
    """(name, keyword arguments of spmm_cg_restated.operator) of calls admm_op_spmm_cg refuses with ADMM_E_INVALID"""
    L = ap._lib
    D, Y = _valid(ap)
    csc = csc_of(D)
    bad_jc = Csc(csc.shape, csc.data, csc.ir, np.concatenate([[1], csc.jc[1:]]))
    unsorted = Csc(csc.shape, csc.data, np.concatenate([csc.ir[1:2], csc.ir[0:1], csc.ir[2:]]), csc.jc)
    rows = [("D is NULL", dict(raw=dict(D=None))), ("Y is NULL", dict(raw=dict(Y=None))),
            ("X is NULL", dict(raw=dict(X=None))), ("state is NULL", dict(raw=dict(state=None))),
            ("K = 0", dict(K=0)), ("K = -1", dict(K=-1)), ("maxit = 0", dict(maxit=0)),
            ("D on the device", dict(D=desc_of(L, csc, mem=L.MEM_DEVICE))),
            ("jc[0] != 0", dict(D=desc_of(L, bad_jc))), ("unsorted rows", dict(D=desc_of(L, unsorted)))]
    rows += [(f"tol = {v}", dict(tol=v)) for v in (0.0, -1e-10, np.inf, np.nan)]
    rows += [(f"shift = {v}", dict(shift=v)) for v in (-1.0, np.inf, np.nan)]
    return rows, (csc, bad_jc, unsorted)


def test_refusals_fire_before_the_device_is_touched(ap):
    """ADMM_E_INVALID with and without a device, every output untouched"""
    L = ap._lib
    assert "admm_op_spmm_cg" in L.EXPORTED_SYMBOLS and hasattr(L.load(), "admm_op_spmm_cg")
    D, Y = _valid(ap)
    assert csc_of(D).jc[1] >= 2 and csc_of(D).ir[0] < csc_of(D).ir[1]  # (the swap of refusal_cases breaks the order inside column 0)
    rows, _keep = refusal_cases(ap)
    for name, kw in rows:
        kw = dict(dict(D=D, shift=1.0), **kw)
        rc, out = R.operator(ap, kw.pop("D"), Y, **kw)
        assert rc == L.E_INVALID, (name, rc, L.load().admm_last_error())
        assert np.isnan(out["X"]).all() and np.isnan(out["R"]).all() and (out["state"] == -1).all(), name
        assert out["next_batch"] == -1, name


def test_no_cpu_fallback(ap):
    """valid arguments: a device's answer, or ADMM_E_DEVICE -- never a host computation"""
    L = ap._lib
    D, Y = _valid(ap)
    rc, out = R.operator(ap, D, Y, shift=1.0)
    msg = L.load().admm_last_error()
    if L.device_count() > 0:
        assert rc == L.OK
    else:
        assert rc == L.E_DEVICE and b"no CPU fallback" in msg
        assert np.isnan(out["X"]).all()
