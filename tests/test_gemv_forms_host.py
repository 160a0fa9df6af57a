"""Which form of the dense product kernels a shape selects (gemv.hip), asked of the planners themselves through
admm_op_gemv_forms -- on the host, no device.  The launchers take other code paths for large matrices: non-temporal
loads (NT = true template instances) above kStreamBytes, and in gemv_t the 4-deep main loop, which a lane enters only
when its chunk holds more than 384 rows, that is with rows_per_chunk >= 512.  tests/test_gpu_gemv_streaming.py runs the
shapes of CASES on the device; this file pins that they select what they are meant to, and that the planner reaches no
template instance / code region the table leaves out.

What the table was derived from (gemv_t_plan): rows_per_chunk starts at 2048 and halves while
ceil(n/32) * ceil(m/rows_per_chunk) < 2048, down to 256.  Because of the ceilings the NT = false main loop IS reachable:
513..768 rows by 32737+ columns (a 134 .. 200 MB matrix) stop at 512 with two row chunks -- 601 x 32771 below -- and a
tall matrix of at most 32 columns (one column tile) stops at 512 from 1 048 065 rows, at 1024 from 2 096 129 and keeps
2048 from 4 192 257, with few enough columns far below kStreamBytes -- 2096649 x 5 below.  And 386+ rows by 65505+
columns keep 2048 with a matrix of 202 MB."""
import ctypes as C

import pytest

# (m, n, rows_per_chunk of gemv_t, nt): the shapes of tests/test_gpu_gemv_streaming.py
CASES = [
    # 206.5 MB.  66 * ceil(m/512) = 1650 < 2048.  m odd, n mod 4 = 1, n mod 32 = 21.  Tail loop and odd row only.
    (12289, 2101, 256, 1),
    # 64 * 33 = 2112 >= 2048 and 64 * 17 < 2048.  Full chunks: exactly one main-loop pass and no tail.  The last chunk
    # has 357 rows: the tail loop and the odd row.
    (16741, 2021, 512, 1),
    # 99 * 21 = 2079 and 99 * 11 = 1089; 527 MB.  Full chunks: two main-loop passes.  The last chunk has 521 rows: one
    # main pass, then lanes 0..3 in the tail loop, then the odd row -- all three regions in one workgroup.
    (21001, 3137, 1024, 1),
    # one chunk of 449 rows under rows_per_chunk = 2048 (2049 column tiles); 235 MB.  Lanes 0..31 take one main pass,
    # lanes 32..63 the tail loop alone, then the odd row; V is staged with the 2048-row stride.
    (449, 65537, 2048, 1),
    # 157.6 MB, below kStreamBytes: the NT = false instance.  1025 column tiles * 2 chunks = 2050 >= 2048.  The full
    # chunk runs one main pass in every lane; the last chunk has 89 rows: the tail loop and the odd row.
    (601, 32771, 512, 0),
    # 84 MB, NT = false, one column tile of 5 columns (the second wave's pass clamps three of its four columns onto
    # the last one, the other two waves have none): 2048 chunks of 1024 rows, where 1024 chunks of 2048 are too few.
    # Full chunks: two main-loop passes; the last chunk has 521 rows: one main pass, lanes 0..3 in the tail loop, the
    # odd row.
    (2096649, 5, 1024, 0),
]

MAIN_LOOP_ROWS = 386  # gemv_t_kernel: `p + 64 * 3 < npairs` holds for lane 0 from npairs = rows / 2 = 193


def forms(L, m, n):
    out = (C.c_int32 * 5)()
    L.check(L.load().admm_op_gemv_forms(m, n, out))
    return dict(zip(("n_nchunk", "n_cols_per_chunk", "t_rows_per_chunk", "t_nchunk", "nt"), out))


def region(f, m):
    """(NT instance, whether any lane of gemv_t enters the 4-deep main loop): what a shape exercises"""
    return f["nt"], int(min(m, f["t_rows_per_chunk"]) >= MAIN_LOOP_ROWS)


@pytest.mark.parametrize("m,n,rc,nt", CASES)
def test_the_streaming_shapes_select_their_forms(ap, m, n, rc, nt):
    f = forms(ap._lib, m, n)
    print(f"{m} x {n}: {f}")
    assert (f["t_rows_per_chunk"], f["nt"]) == (rc, nt), f
    assert (8 * m * n > 192 << 20) == bool(nt)
    assert f["t_nchunk"] == -(-m // rc)
    assert f["n_nchunk"] * f["n_cols_per_chunk"] >= n > (f["n_nchunk"] - 1) * f["n_cols_per_chunk"]


def test_the_table_reaches_every_region_it_claims(ap):
    """per case the rows of a full chunk and of the last one, as the comments of CASES state them"""
    passes = lambda rows: len(range(0, max(0, rows // 2 - 192), 256))  # main-loop passes of lane 0
    full = {(m, n): passes(min(m, rc)) for m, n, rc, _ in CASES}
    last = {(m, n): (m - (m - 1) // rc * rc) for m, n, rc, _ in CASES}
    assert full == {(12289, 2101): 0, (16741, 2021): 1, (21001, 3137): 2, (449, 65537): 1, (601, 32771): 1,
                    (2096649, 5): 2}
    assert last == {(12289, 2101): 1, (16741, 2021): 357, (21001, 3137): 521, (449, 65537): 449, (601, 32771): 89,
                    (2096649, 5): 521}
    assert passes(521) == 1 and 521 // 2 - 256 == 4  # one main pass, then lanes 0..3 in the tail loop
    assert all(m % 2 == 1 for m, _, _, _ in CASES)   # every last chunk ends in the odd row


def test_the_operator_tests_of_test_gpu_ops_stay_in_the_small_form(ap):
    """every shape of test_gemv_t / test_gemv_n selects rows_per_chunk = 256 and plain loads: the tail loop and the odd
    row are all they run"""
    import test_gpu_ops

    for test in (test_gpu_ops.test_gemv_t, test_gpu_ops.test_gemv_n):
        (mark,) = [k for k in test.pytestmark if k.name == "parametrize"]
        assert len(mark.args[1]) >= 7
        for m, n, *_ in mark.args[1]:
            f = forms(ap._lib, m, n)
            assert (f["t_rows_per_chunk"], f["nt"]) == (256, 0), (m, n, f)
            assert region(f, m) == (0, 0)


def test_no_reachable_region_is_left_out_of_the_table(ap):
    """over a coarse grid of shapes up to 2^26 elements (512 MB): every (NT instance, main loop entered or not) and
    every rows_per_chunk the planner selects is run by test_gpu_ops (256, plain loads, no main loop) or by a shape of
    CASES.  A planner or kStreamBytes change that makes another combination reachable fails here and names it."""
    L = ap._lib
    covered = {(0, 0)} | {region(forms(L, m, n), m) for m, n, _, _ in CASES}
    covered_rc = {256} | {rc for _, _, rc, _ in CASES}
    side = sorted({v for a in range(27) for v in (1 << a, (1 << a) + 1, (1 << a) - 1, 3 << a >> 1) if v >= 1})
    seen, plain_main = 0, []
    for m in side:
        for n in side:
            if m * n > 1 << 26:
                break
            f = forms(L, m, n)
            seen += 1
            assert region(f, m) in covered, f"{m} x {n} selects {f}: (nt, main loop) = {region(f, m)} is not tested"
            assert f["t_rows_per_chunk"] in covered_rc, f"{m} x {n} selects {f}: that rows_per_chunk is not tested"
            if region(f, m) == (0, 1):
                plain_main.append((m, n, f["t_rows_per_chunk"]))
    assert seen > 3000
    # the NT = false main loop is reachable: wide matrices at 512, tall and narrow ones at every rows_per_chunk
    assert (513, 32768, 512) in plain_main and ((1 << 19) - 1, 33, 512) in plain_main
    assert {rc for _, _, rc in plain_main} == {512, 1024, 2048}


def test_gemv_forms_refuses_bad_arguments(ap):
    L = ap._lib
    out = (C.c_int32 * 5)()
    for m, n, o in ((0, 4, out), (4, 0, out), (-1, 4, out), (4, 4, None), (1 << 21, 1 << 20, out)):
        assert L.load().admm_op_gemv_forms(m, n, o) == L.E_INVALID
    assert "admm_op_gemv_forms" in L.EXPORTED_SYMBOLS
