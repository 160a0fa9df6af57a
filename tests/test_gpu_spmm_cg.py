"""The lock-step CG of the sparse multi-fit solvers on the device, alone: one call of admm_op_spmm_cg per
case -- SpmmCg::solve and the kernels of spmm_cg.hip as a run drives them -- against the NumPy restatement of the same
recurrence (spmm_cg_restated): the counters against the float64 one, x against the longdouble one.

Bounds.  X_BOUND, DRIFT_BOUND and R_BOUND are 10x what test_spmm_cg_host measures between the float64 and the longdouble
restatement over these very cases (2.2e-10, 2.2e-15 and 1.2e-14); the factor is the project's margin for the device's
summation order inside the products.  An iteration count is compared only where the stop test cannot flip
(spmm_cg_restated.guard, checked there on the CPU for every fit of every case).  The padding columns of the chunked
buffers and a frozen fit's X, R, P and state are checked by the operator itself: a call that returns 0 has passed them.

The exits this file reaches and the whole-run tests of test_gpu_sparse_*.py do not: p.q = 0 (brk), a zero right-hand side
behind a warm start, done at the start, a last batch shorter than the others, a frozen fit's R and P."""
import numpy as np
import pytest

import spmm_cg_restated as R
from test_spmm_cg_host import refusal_cases

pytestmark = pytest.mark.gpu

LD = np.longdouble
COUNTERS = ("iters", "capped", "brk", "zero")


def _check_fit(ap, name, got, k, counts=True):
    """fit k of a call on the inputs of case `name` against its restatement"""
    c = R.inputs(ap, name)
    case, y = c["case"], c["Y"][:, k]
    f64, ld = R.restated(ap, name, np.float64)[k], R.reference(ap, name)[k]
    x, r = got["X"][:, k], got["R"][:, k]
    state = {f: int(got[f][k]) for f in R.STATE}
    assert not np.isnan(x).any() and not np.isnan(r).any(), (name, k)
    assert state["done"] == 1 and state["total"] == state["iters"], (name, k, state)
    if counts:
        assert [state[f] for f in COUNTERS] == [f64[f] for f in COUNTERS], (name, k, state, [f64[f] for f in COUNTERS])
    xinf = float(np.max(np.abs(ld["x"])))
    gap = float(np.max(np.abs(x.astype(LD) - ld["x"])))
    ynorm = float(np.linalg.norm(y))
    rt = R.true_residual(c["A"], y, x, case.shift)
    rtn, rn = float(np.linalg.norm(rt)), float(np.linalg.norm(r.astype(LD)))
    rgap = float(np.linalg.norm(r.astype(LD) - rt))
    print(f"{name}, fit {k}: {state}, x gap {gap / xinf if xinf else gap:.3e} (bound {R.X_BOUND:.1e}), "
          f"||r_true|| / ||y|| {rtn / ynorm if ynorm else rtn:.3e}, | ||R|| - ||r_true|| | / ||y|| "
          f"{abs(rn - rtn) / ynorm if ynorm else 0.0:.3e} (bound {R.DRIFT_BOUND:.1e}), ||R - r_true|| / ||y|| "
          f"{rgap / ynorm if ynorm else 0.0:.3e} (bound {R.R_BOUND:.1e})")
    assert gap <= R.X_BOUND * xinf, (name, k, gap, xinf)
    if state["zero"]:
        return
    if state["capped"] == 0:
        assert rtn <= case.tol * ynorm + R.DRIFT_BOUND * ynorm, (name, k, rtn / ynorm)
    assert abs(rn - rtn) <= R.DRIFT_BOUND * ynorm, (name, k, abs(rn - rtn) / ynorm)
    assert rgap <= R.R_BOUND * ynorm, (name, k, rgap / ynorm)


def _check_case(ap, name, got, counts=True):
    for k in range(len(R.CASES[name].fits)):
        _check_fit(ap, name, got, k, counts)


def _same_bits(a, b, cols_a=slice(None), cols_b=slice(None)):
    return (np.array_equal(a["X"][:, cols_a].view(np.uint64), b["X"][:, cols_b].view(np.uint64))
            and np.array_equal(a["R"][:, cols_a].view(np.uint64), b["R"][:, cols_b].view(np.uint64))
            and np.array_equal(a["state"][cols_a], b["state"][cols_b]))


# ------------------------------------------------------------------------------------------------ iterate parity
@pytest.mark.parametrize("name", ["A65 shift 0", "A65 shift 1", "A65 shift 2.5", "FAT shift 0", "FAT shift 1",
                                  "FAT shift 2.5"])
def test_iterates_against_the_restatement(gpu, name):
    """shift 0 (the SHIFT = false kernels) and 1, 2.5 (SHIFT = true) on the same matrices, K = 3, 11, 21, 1, 3, 10"""
    assert R.CASES[name].tol == 1e-10
    _check_case(gpu, name, R.run_case(gpu, name))


def test_iterates_of_ordinary_right_hand_sides_without_a_shift(gpu):
    """45 to 49 iterations at cond 390: everything but the count, which rounding alone moves by two (spmm_cg_restated)"""
    name = "A65 shift 0 generic"
    got = R.run_case(gpu, name)
    assert (got["capped"] == 0).all() and (got["iters"] > 40).all()
    _check_case(gpu, name, got, counts=False)


@pytest.mark.parametrize("name", [f"n = {n} shift {s}" for n in (1, 31, 32, 33) for s in (0, 1)]
                         + ["WIDE shift 0", "WIDE shift 2.5"])
def test_row_block_edges(gpu, name):
    """one row, a row block less one, exactly one, one more; 8300 > 32 * 256: a workgroup takes a second row block"""
    case = R.CASES[name]
    n = R.matrix(gpu, case.shape).shape[1]
    if name.startswith("WIDE"):
        assert n > 32 * 256 and len(case.fits) == 3
    else:
        assert n in (1, 31, 32, 33) and len(case.fits) == 11
    _check_case(gpu, name, R.run_case(gpu, name), counts=case.counts)  # (no count for n > 1 without a shift)


# ------------------------------------------------------------------------------------------------ independence
def test_a_fit_has_the_same_bits_wherever_it_lands(gpu):
    """K = 21, the same right-hand side in fits 0, 10 and 20 (three chunks, the last one of a single fit): bit-equal to
    one another and to the fit run alone; a second call returns the same bits"""
    c = R.inputs(gpu, "same three")
    assert np.array_equal(c["Y"][:, 0], c["Y"][:, 10]) and np.array_equal(c["Y"][:, 0], c["Y"][:, 20])
    got = R.run_case(gpu, "same three")
    _check_case(gpu, "same three", got)
    for k in (10, 20):
        assert _same_bits(got, got, [0], [k]), k
    case = c["case"]
    rc, alone = R.operator(gpu, c["D"], c["Y"][:, :1], shift=case.shift, tol=case.tol, maxit=case.maxit)
    gpu._lib.check(rc)
    assert _same_bits(got, alone, [0], [0])
    assert _same_bits(got, R.run_case(gpu, "same three"))


# ------------------------------------------------------------------------------------------------ the exits
def test_exit_without_a_division(gpu):
    """y = e_7, the empty column, without a shift: D p = 0, p.q = 0 -- brk, one iteration, counted as capped, x as it was"""
    got = R.run_case(gpu, "brk")
    assert [int(got[f][1]) for f in R.STATE] == [1, 1, 1, 1, 1, 0]
    assert not got["X"][:, 1].any()
    _check_case(gpu, "brk", got)  # (the neighbours too)
    warm = R.run_case(gpu, "brk warm")
    X0 = R.inputs(gpu, "brk warm")["X0"]
    assert X0[R.EMPTY_COLUMN, 1] == 0.75 and [int(warm[f][1]) for f in R.STATE] == [1, 1, 1, 1, 1, 0]
    assert np.array_equal(warm["X"][:, 1].view(np.uint64), X0[:, 1].view(np.uint64))
    _check_case(gpu, "brk warm", warm)


def test_empty_column_with_a_shift(gpu):
    """the same y with shift 2: x_7 = 1 / 2 after one iteration, every other entry 0.0, converged"""
    got = R.run_case(gpu, "e7 shift 2")
    assert [int(got[f][1]) for f in R.STATE] == [1, 1, 0, 1, 0, 0]
    x = got["X"][:, 1]
    assert x[R.EMPTY_COLUMN] == 0.5 and np.count_nonzero(x) == 1
    _check_case(gpu, "e7 shift 2", got)


@pytest.mark.parametrize("name", ["zero", "zero warm"])
def test_zero_right_hand_side(gpu, name):
    """x = 0.0 exactly, no iteration, not capped -- from x = 0 and behind a warm start that is not zero"""
    c = R.inputs(gpu, name)
    assert not c["Y"][:, 1].any() and (c["X0"] is None or c["X0"][:, 1].any())
    got = R.run_case(gpu, name)
    assert [int(got[f][1]) for f in R.STATE] == [0, 0, 0, 1, 0, 1]
    assert not got["X"][:, 1].any() and not np.signbit(got["X"][:, 1]).any()
    _check_case(gpu, name, got)


def test_converged_warm_start(gpu):
    """the x of a solve at tol = 1e-13 under tol = 1e-8: done at the start, x bit for bit"""
    first = R.run_case(gpu, "tight")
    _check_case(gpu, "tight", first, counts=False)
    assert (first["capped"] == 0).all() and (first["iters"] > 9).all()
    case = R.CASES["converged"]
    assert (case.tol, R.CASES["tight"].tol) == (1e-8, 1e-13)
    got = R.run_case(gpu, "converged", X0=first["X"])
    K = len(case.fits)
    for f, v in zip(R.STATE, (0, 0, 0, 1, 0, 0)):
        assert (got[f] == v).all(), (f, got[f])
    assert got["X"].shape == (65, K) and np.array_equal(got["X"].view(np.uint64), first["X"].view(np.uint64))


def test_mixed_finish_inside_a_chunk(gpu):
    """fit 0 is done after one iteration, its nine neighbours run on for more than 20: masked products, a stale Q"""
    got = R.run_case(gpu, "mixed")
    assert int(got["iters"][0]) == 1 and (got["iters"][1:] > 20).all()
    _check_case(gpu, "mixed", got)


# ------------------------------------------------------------------------------------------------ the cap and the batch
@pytest.mark.parametrize("batch", [4, 0])
@pytest.mark.parametrize("maxit", [1, 3, 5, 9])
def test_cap_and_batch(gpu, maxit, batch):
    """maxit inside the first batch (1, 3 under both; 5 under the default 8), at a short last batch (5 = 4 + 1,
    9 = 4 + 4 + 1 = 8 + 1): every fit stops at exactly maxit iterations with the restatement's iterate"""
    name = f"maxit {maxit}"
    got = R.run_case(gpu, name, batch=batch)
    assert (got["iters"] == maxit).all() and (got["capped"] == 1).all() and (got["done"] == 1).all()
    _check_case(gpu, name, got)
    if batch <= 0:
        assert got["next_batch"] == min(64, max(4, maxit + 2))


def test_batch_follows_the_longest_fit(gpu):
    got = R.run_case(gpu, "mixed")
    assert got["next_batch"] == min(64, max(4, int(got["iters"].max()) + 2)) and got["next_batch"] > 22


# ------------------------------------------------------------------------------------------------ a frozen fit
def test_frozen_fit(gpu):
    """K = 11, fits 4 and 10 stopped (10 alone in the last chunk): the call succeeds -- the operator found their X, R, P
    and state untouched -- and the other nine have the bits of the call without stop"""
    name = "A65 shift 1"
    free = R.run_case(gpu, name)
    stop = np.zeros(11, dtype=np.int32)
    stop[[4, 10]] = 1
    got = R.run_case(gpu, name, stop=stop)
    assert not got["state"][[4, 10]].any()
    run = [k for k in range(11) if k not in (4, 10)]
    assert _same_bits(got, free, run, run)
    for k in run:
        _check_fit(gpu, name, got, k)
    warm = R.run_case(gpu, name, stop=stop, X0=0.5 * free["X"])  # (the products in front of a warm start skip them too)
    assert not warm["state"][[4, 10]].any() and (warm["done"][run] == 1).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_process_able_to_solve(gpu):
    L = gpu._lib
    c = R.inputs(gpu, "A65 shift 1")
    rows, _keep = refusal_cases(gpu)
    for name, kw in rows:
        kw = dict(dict(D=c["D"], shift=1.0), **kw)
        rc, _ = R.operator(gpu, kw.pop("D"), c["Y"][:, :3], **kw)
        assert rc == L.E_INVALID, (name, rc)
        rc, out = R.operator(gpu, c["D"], c["Y"][:, :3], shift=1.0)
        assert rc == L.OK, (name, L.load().admm_last_error())
        for k in range(3):
            _check_fit(gpu, "A65 shift 1", out, k)
