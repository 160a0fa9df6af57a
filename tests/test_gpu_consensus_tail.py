"""The exchange and update kernels of consensus lasso (consensus.hip: cons_sum_kernel, cons_gather_sum_kernel,
cons_update_kernel, cons_gather_update_kernel<64, 16>) through admm_op_consensus_tail, one operator call per case,
against the long-double restatement of tests/consensus_restated.py.

Two kinds of input:

int    rows, U, D's, xave, ubar are integers in +-2^20, rho = 2, lambda = 2^22: every gathered sum is an integer far below
       2^53 and exact in ANY order, so X and `sums` must equal the int64 reference bit for bit.  A skipped, doubled or
       mis-sourced partial row fails with certainty (a row from outside the placement is NaN).  Three elements sit
       exactly on the kink of the soft threshold (v = +t, -t, 0).
real   standard-normal data; partial rows 0 and 1 of every slice cancel to 1e-8.  X is held to the any-order summation
       bound (P - 1) * 2^-53 * sum_p |rows[k][p][i]|, per element.

What follows the gather is checked from the x_k the call itself returned (for integer rows that IS the reference): the
restatement evaluates the tail in long double from those x_k, and z, U, Y, xave, ubar must lie within
16 * 2^-53 * max(|x_k|, |u_k|, |z|, |D's|) of it (the maximum over the slices of every rank, * max(1, rho) for Y).  The
kernels put at most eight fp64 roundings between the operands and any of these values (the slice sums of real data
aside, whose roundings average out at a small fraction of an ulp of the mean); the factor 2 is the margin, and
tests/test_consensus_tail_host.py shows a float64 evaluation in kernel order uses at most 0.359 of the bound.

The five slot sums and q are reductions of vectors the same call returned, each of which is bounded above, so they are
compared with math.fsum over exactly those vectors: relative error <= n * K * 2^-52, the worst case of a sum of
non-negative terms in any order plus the roundings of a term.  (Comparing with the sums of the REFERENCE's vectors would
fold the vectors' own admissible errors into the sums, amplified by the cancellation in ubar = v - z.)

Out of reach here: the tile-striding loop of cons_gather_update_kernel beyond 1024 workgroups needs n > 65536, hundreds
of MB of partial rows per call.
"""
import functools

import numpy as np
import pytest

import consensus_restated as CR

pytestmark = pytest.mark.gpu

LD = np.longdouble
U53 = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _case(form, K, n, kind, Ntot=None):
    case = CR.make_case(form, K, n, kind, Ntot)
    if form != 0:
        case["X64"], case["XLD"] = CR.assemble(case["rows"])  # once per case, shared by every test that uses it
    else:
        case["X64"], case["XLD"] = case["X"].astype(np.float64), case["X"].astype(LD)
    return case


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _run(gpu, case, form=None, with_q=0):
    form = case["form"] if form is None else form
    rc, got = CR.call_tail(gpu._lib.load(), gpu._lib.as_dp, form, case["n"], case["K"], case["Ntot"], case["rho"],
                           case["lam"], None if form == 0 else case["rows"], case["X64"] if form == 0 else None,
                           case["U"], case["Dts"], case["xave"], case["ubar"], case["remote"], with_q)
    gpu._lib.check(rc)
    return got


def _check(gpu, case, with_q=0):
    form, K, n, kind = case["form"], case["K"], case["n"], case["kind"]
    tag = f"form {form} K {K} n {n} {kind} q {with_q}"
    got = _run(gpu, case, with_q=with_q)
    for name in ("X", "U", "Y", "z", "xave", "xaveprev", "ubar", "slots"):
        assert not np.any(np.isnan(got[name])), f"{tag}: NaN in {name}"
    # ---- the gather
    if kind == "int" or form == 0:
        np.testing.assert_array_equal(got["X"], case["X64"], err_msg=tag)
    else:
        bound = (case["P"] - 1) * LD(U53) * np.abs(case["rows"]).astype(LD).sum(axis=1)
        ratio = float(np.max(np.abs(got["X"].astype(LD) - case["XLD"]) / bound))
        print(f"{tag}: X error / summation bound = {ratio:.3f}")
        assert ratio <= 1.0, tag
    ref = CR.consensus_tail(got["X"], case["U"], case["Dts"], case["xave"], case["ubar"], case["rho"], case["lam"],
                            case["Ntot"], remote=case["remote"], sums=False)
    if form == 2:
        assert CR.is_sentinel(got["sums"]), f"{tag}: the one-launch tail stores no sums"
    elif kind == "int":
        np.testing.assert_array_equal(got["sums"], ref["sums"].astype(np.float64), err_msg=tag)
    else:
        mag = np.stack([np.abs(got["X"]).astype(LD).sum(axis=0), np.abs(case["U"]).astype(LD).sum(axis=0)])
        if case["remote"] is not None:
            mag = mag + np.abs(case["remote"]).astype(LD)
        assert np.all(np.abs(got["sums"].astype(LD) - ref["sums"]) <= K * LD(U53) * mag), tag
    # ---- the element update
    ratios = CR.vector_ratios(case, got, ref, got["X"])
    print(f"{tag}: error / 16-rounding bound = " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, (tag, ratios)
    assert np.array_equal(_bits(got["xaveprev"]), _bits(case["xave"])), tag
    margin = 16 * LD(U53) * CR.operand_scale(case, got["X"], ref["z"])
    av = np.abs(ref["v"])
    assert np.all(got["z"][av <= ref["t"] - margin] == 0), f"{tag}: z is not zero inside the threshold"
    assert np.all(got["z"][av > ref["t"] + margin] != 0), f"{tag}: z is zero outside the threshold"
    for i, target in case["kinks"].items():
        assert got["z"][i] == 0 and np.signbit(got["z"][i]) == (target < 0), f"{tag}: element {i} on the kink"
    # ---- the reductions, of the vectors this call returned
    sums = CR.slot_sums(got["X"], got["xave"], got["xaveprev"], got["ubar"], case["ubar"],
                        center=case["xave"] if with_q else None)
    rel = n * K * 2.0 ** -52
    pairs = [(name, got["slots"][j], sums[name]) for j, name in enumerate(CR.SLOT_NAMES)]
    if with_q:
        assert not np.isnan(got["q"][0]), tag
        pairs.append(("q", got["q"][0], sums["q"]))
    else:
        assert CR.is_sentinel(got["q"]), f"{tag}: q written without with_q"
    for name, g, r in pairs:
        assert abs(LD(g) - r) <= rel * r, f"{tag}: {name} = {g!r}, fsum {float(r)!r}, allowed relative error {rel:.3e}"
    return got


KINDS = ("int", "real")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", [K for _, K, _ in CR.F2_K_SWEEP])
def test_one_launch_tail_slot_dealing(gpu, K, kind):
    """cons_gather_update_kernel at n = 1537 (P = 14 rows, a ragged last 64-tile): SUB = 16 / K row ranges per slice =
    16, 8, 5, 3, 2, 2, 1, 1, 1; K = 3, 5, 7, 9, 15 leave whole slots idle, K = 3, 5, 7 give ranges of unequal length and
    K = 1, 2 ranges that start at or past P.  Catches `per` rounded down (rows past SUB * per are never read), a wrong
    kk / sb split, an idle slot that stores."""
    _check(gpu, _case(2, K, 1537, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", sorted({n for _, _, n in CR.F2_N_SWEEP}))
@pytest.mark.parametrize("K", [3, 16])
def test_one_launch_tail_sizes(gpu, K, n, kind):
    """Ragged and exact 64-tiles, ragged and exact 128-tiles of the x-solve (d = ic / 128 picks the N- or the T-part row:
    `pq <= d` -> `pq < d` takes the diagonal row from the T-part, which holds NaN there), one element, several
    workgroups.  A store past n (`i <= n`) lands in the next slice's X or in the padding and shows as a changed x_k."""
    _check(gpu, _case(2, K, n, kind))


@pytest.mark.parametrize("K,n,kind", [(K, n, kind) for _, K, n in CR.F2_ROUND2 for kind in KINDS] +
                         [CR.F2_BENCH[1:] + ("int",)])
def test_one_launch_tail_second_round_of_row_loads(gpu, K, n, kind):
    """More than kCgRows = 20 rows in one slot's range: (9, 2433) P = 21, one row in round two; (16, 2561) P = 22, two;
    (8, 5121) per = 21 for both ranges of a slice; (5, 7553) P = 61, per = 21 over three ranges; (8, 10000) the
    benchmark's own dealing, two full rounds.  Catches a dropped second round and a wrong clamp `pq = p1 - 1`."""
    _check(gpu, _case(2, K, n, kind))


@pytest.mark.parametrize("with_q", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,n", [(K, n) for _, K, n in CR.F1_SHAPES])
def test_two_launch_tail_from_partial_rows(gpu, K, n, kind, with_q):
    """cons_gather_sum_kernel + cons_update_kernel: K past the 16 slots of the one-launch form (17, 33), P = 3 and 5 where
    the fourth slot starts at p0 >= P, per = 21 at n = 10113 (a second round of one row), with and without the q of the
    sharded run (centre = the xave that came in: ignoring it changes q)."""
    _check(gpu, _case(1, K, n, kind), with_q)


@pytest.mark.parametrize("with_q", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,n", [(K, n) for _, K, n in CR.F0_SHAPES])
def test_two_launch_tail_from_stored_x(gpu, K, n, kind, with_q):
    """cons_sum_kernel + cons_update_kernel on x_k in memory; n = 70001 takes both grid-stride loops several times"""
    _check(gpu, _case(0, K, n, kind), with_q)


@pytest.mark.parametrize("with_q", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", [0, 1])
def test_tail_with_slices_on_other_ranks(gpu, form, kind, with_q):
    """K = 3 local slices of Ntot = 7, the other four as the `remote` share of the sums: the means divide by 7 and the
    threshold is lambda / (rho * 7) -- a tail that uses K fails z, xave and everything behind them"""
    _check(gpu, _case(form, 3, 1537, kind, 7), with_q)


@pytest.mark.parametrize("K,n", [(3, 1537), (16, 129), (9, 2433)])
def test_forms_agree_bit_for_bit_on_integer_rows(gpu, K, n):
    """Once x_k is exact the three launch sequences evaluate the same fp64 expressions: X, z, U, Y, xave, ubar are
    identical bit for bit (rho = 2 makes the product in y_k exact, so a fused multiply-add changes nothing)."""
    case = _case(2, K, n, "int")
    runs = [_run(gpu, case, form) for form in (0, 1, 2)]
    for name in ("X", "z", "U", "Y", "xave", "ubar", "xaveprev"):
        for form in (1, 2):
            assert np.array_equal(_bits(runs[0][name]), _bits(runs[form][name])), (name, form)


@pytest.mark.parametrize("form", [0, 1, 2])
def test_tail_is_reproducible(gpu, form):
    """two calls, identical bits: every vector, the slot sums, q"""
    case = _case(max(form, 1), 5, 1537, "real")
    with_q = 0 if form == 2 else 1
    a, b = _run(gpu, case, form, with_q), _run(gpu, case, form, with_q)
    for name in a:
        assert np.array_equal(_bits(a[name]), _bits(b[name])), name
