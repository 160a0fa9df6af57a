"""The 40-bit width of the compact x-solve storage (csrc/tri_tile.h: off-diagonal 128 x 128 tiles as 40-bit fixed point
with one power-of-two scale per tile -- a signed hi byte and an unsigned lo dword per element --, diagonal tiles fp64)
against a NumPy model of the format written here, through admm_op_symv_compact_bits (pack kernel + compact product),
and through the engine, which tries this width first once even the 48-bit store is larger than kSymvCacheBytes.

No measured tolerance, as in test_gpu_symv_compact.py: the dequantised matrix is compared bit for bit, the product with
the summation bound (k + 4) * 2^-53 * |Q||x| against a longdouble reference, the distance to the unquantised matrix
with the bound the format gives: half a unit of the tile's scale per element, a whole unit where the clamp acts (an
element v with 2^e - scale / 2 <= |v| < 2^e rounds to 2^39 units and is stored as 2^39 - 1).

Fault injection (each on a scratch copy of the sources, never committed; the assertion that caught it):
  (a) hi zero-extended instead of sign-extended (SyBufCq::hi_field), run on the device: `y = Q x inside the summation
      bound` of test_compact40_product_against_the_model fails in 19 of its 20 cases (|y - Qx| of a few hundred against
      a bound of 3e-10); "zero" at n = 129 passes, its only off-diagonal tile is all zero.  The dequantised matrix,
      which the pack kernel writes, stays right;
  (c) scale exponent off by one (2^(e - 38) in the pack kernel), run on the device: `dequantised matrix differs`, the
      same 19 cases;
  (b) tile offset (3 t + bi) * 32 KB in place of (5 t + 3 bi) * 16 KB: NOT run on the device.  The pack kernel, the
      product, the allocation and the byte counts share cq_tile_offset, so the mistake there gives a consistent,
      larger store: the operator cases pass and `stored_bytes == nt * 8 T^2 + (ntri - nt) * 5 T^2` of the engine test
      fails (host arithmetic: (3 ntri + nt) * 32 KB instead).  The mistake in the product alone reads past the end of
      the store from tile 2 on; an out-of-bounds read is not something to run."""
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
T = 128
BITS = 40
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ===================================================================================== the model
def quantise_model(S, bits=BITS):
    """(Q, H): Q = the symmetric matrix the compact storage of S's lower triangle stands for; H[i, j] = the largest
    error the format allows in element (i, j): 2^(e - bits), half a unit, in an off-diagonal tile whose largest
    magnitude is < 2^e -- a whole unit where the clamp acts --, 0 in diagonal tiles and in all-zero tiles."""
    n = S.shape[0]
    nt = -(-n // T)
    P = np.zeros((nt * T, nt * T))
    P[:n, :n] = np.tril(S)
    Q = P.copy()
    H = np.zeros_like(P)
    lim = 2.0 ** (bits - 1) - 1
    for bi in range(nt):
        for bj in range(bi):
            blk = P[bi * T:(bi + 1) * T, bj * T:(bj + 1) * T]
            mx = np.max(np.abs(blk))
            if mx == 0.0:
                continue  # scale 0, zeros
            _, e = np.frexp(mx)  # mx = f * 2^e, f in [0.5, 1)
            r = np.rint(np.ldexp(blk, bits - 1 - int(e)))
            Q[bi * T:(bi + 1) * T, bj * T:(bj + 1) * T] = np.ldexp(np.clip(r, -lim, lim), int(e) - (bits - 1))
            H[bi * T:(bi + 1) * T, bj * T:(bj + 1) * T] = np.where(np.abs(r) > lim, 2.0, 1.0) * 2.0 ** (int(e) - bits)
    Q, H = Q[:n, :n], H[:n, :n]
    return np.tril(Q) + np.tril(Q, -1).T, np.tril(H) + np.tril(H, -1).T


KINDS = ("plain", "pow2", "zero", "span32", "negmax")


@functools.lru_cache(maxsize=None)
def _case(n, kind):
    """(S, x, Q, H, refQ, boundQ, refS): S symmetric with a dominant diagonal; `kind` reshapes the LAST off-diagonal
    tile of the first tile column (the only one at n = 129, where it is one live row and 127 rows of padding)."""
    rng = np.random.default_rng(9000 * n + KINDS.index(kind))
    low = np.tril(rng.standard_normal((n, n)))
    low[np.diag_indices(n)] += 300.0 * (1.0 + rng.random(n))  # hundreds of times the rest of its tile
    nt = -(-n // T)
    r0 = (nt - 1) * T
    blk = low[r0:, :T]  # a view: tile (nt - 1, 0)
    if kind == "pow2":  # the tile's maximum is exactly 2^-3: e = -2, one binade above its other entries' exponent
        blk *= 0.1 / np.max(np.abs(blk))
        blk[0, 5] = 0.125
    elif kind == "zero":
        blk[:] = 0.0
    elif kind == "span32":  # magnitudes 2^-32 .. 1 under a maximum of 1.5: the grid is 2^-38, small entries become 0
        blk *= np.ldexp(1.0 / np.max(np.abs(blk)), -rng.integers(0, 33, blk.shape))
        blk[0, 0], blk[-1, -1] = 1.5, 1.5 * 2.0 ** -40  # (the last one is 3/8 of a unit: stored as 0)
    elif kind == "negmax":  # the maximum is negative and rounds to -2^39 units: clamped to -(2^39 - 1), hi byte 0x80
        blk *= 4.0 / np.max(np.abs(blk))
        blk[-1, 77] = -8.0 * (1.0 - 2.0 ** -41)
    S = low + np.tril(low, -1).T
    x = rng.standard_normal(n)
    Q, H = quantise_model(S)
    xl = x.astype(LD)
    refQ = Q.astype(LD) @ xl
    boundQ = (n + 4) * LD(U) * (np.abs(Q).astype(LD) @ np.abs(xl))
    refS = S.astype(LD) @ xl
    for a in (S, x, Q, H, refQ, boundQ, refS):
        a.setflags(write=False)
    return S, x, Q, H, refQ, boundQ, refS


def _lower_storage(S):
    M = np.asfortranarray(S.copy())
    M[np.triu_indices(S.shape[0], 1)] = np.nan  # the kernels read the lower triangle only
    return M


def _op(gpu, M, n, x, fin, ncached, parts, want_q=False, bits=BITS):
    dp = gpu._lib.as_dp
    y = np.full(n, np.nan)
    Q = np.full((n, n), np.nan, order="F") if want_q else None
    gpu._lib.check(gpu._lib.load().admm_op_symv_compact_bits(dp(M), n, M.shape[0], dp(x), fin, ncached, parts, dp(y),
                                                             dp(Q) if want_q else None, n, bits))
    return (y, Q) if want_q else y


def _tiles(n):
    t = -(-n // T)
    return t * (t + 1) // 2


def test_the_cases_hold_what_they_are_for():
    """properties of the inputs themselves (model only): the clamp acts in "negmax" and leaves hi = -128, entries of
    "span32" fall below the grid, the maximum of "pow2" sits on a power of two"""
    n, r0 = 300, 256
    S, _, Q, H, *_ = _case(n, "negmax")
    assert Q[r0 + 43, 77] == -(2.0 ** 39 - 1) * 2.0 ** -36 and S[r0 + 43, 77] < Q[r0 + 43, 77]
    assert H[r0 + 43, 77] == 2.0 ** -36 and H[r0, 0] == 2.0 ** -37
    S, _, Q, *_ = _case(n, "span32")
    blkS, blkQ = S[r0:, :T], Q[r0:, :T]
    assert blkQ[-1, -1] == 0.0 and np.count_nonzero((blkQ == 0.0) & (blkS != 0.0)) >= 1
    assert np.max(np.abs(blkS)) == 1.5
    S, _, Q, *_ = _case(n, "pow2")
    assert np.max(np.abs(S[r0:, :T])) == 0.125 and Q[r0, 5] == 0.125


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [129, 300, 1000, 1664])
def test_compact40_product_against_the_model(gpu, n, kind):
    """The matrix the kernel multiplied is the model's bit for bit (pack kernel: exponent, rounding, clamp, the hi / lo
    split, the layout as the product kernel reads it back); y = Q x inside the summation bound, the same bits for
    every cache split and with or without the finalize passenger; inside the format's bound of the unquantised S x;
    three dealt parts add up inside the same bounds.  One part runs on NaN-filled partial slots."""
    S, x, Q, H, refQ, boundQ, refS = _case(n, kind)
    M = _lower_storage(S)
    y0, Qg = _op(gpu, M, n, x, 0, -1, 1, want_q=True)
    assert np.array_equal(Qg.view(np.uint64), np.asfortranarray(Q).view(np.uint64)), "dequantised matrix differs"
    if kind == "zero":
        assert not Qg[(-(-n // T) - 1) * T:, :T].any()
    fmt = H.astype(LD) @ np.abs(x).astype(LD)  # sum_j (1 or 2) * 2^(e_tile(i, j) - 40) |x_j|
    worst = 0.0
    for fin in (0, 1):
        for nc in (0, _tiles(n), -1):
            for parts in (1, 3):
                y = _op(gpu, M, n, x, fin, nc, parts)
                assert not np.isnan(y).any(), (fin, nc, parts)
                eq = np.abs(y.astype(LD) - refQ)
                es = np.abs(y.astype(LD) - refS)
                worst = max(worst, float(np.max(eq / boundQ)))
                assert np.all(eq <= boundQ), (fin, nc, parts, float(np.max(eq / boundQ)))
                assert np.all(es <= fmt + boundQ), (fin, nc, parts)
                if parts == 1:
                    assert np.array_equal(y.view(np.uint64), y0.view(np.uint64)), (fin, nc)
    print(f"symv_compact40 n={n} {kind}: worst |y - Qx| / bound = {worst:.3f}, "
          f"max |y - Sx| / (format bound + summation bound) = {float(np.max(es / (fmt + boundQ))):.3f}")


@pytest.mark.parametrize("n", [129, 1000])
def test_48_bits_through_the_new_entry_is_admm_op_symv_compact(gpu, n):
    S, x, *_ = _case(n, "negmax")
    M = _lower_storage(S)
    lib, dp = gpu._lib.load(), gpu._lib.as_dp
    for fin, parts in ((0, 1), (1, 1), (0, 3)):
        y_old, Q_old = np.full(n, np.nan), np.full((n, n), np.nan, order="F")
        gpu._lib.check(lib.admm_op_symv_compact(dp(M), n, n, dp(x), fin, -1, parts, dp(y_old), dp(Q_old), n))
        y_new, Q_new = _op(gpu, M, n, x, fin, -1, parts, want_q=True, bits=48)
        assert not np.isnan(y_new).any() and not np.isnan(Q_new).any()
        assert np.array_equal(y_new.view(np.uint64), y_old.view(np.uint64)), (fin, parts)
        assert np.array_equal(Q_new.view(np.uint64), Q_old.view(np.uint64)), (fin, parts)


def test_other_widths_and_bad_arguments_are_refused(gpu):
    S, x, *_ = _case(129, "plain")
    M = _lower_storage(S)
    lib, dp = gpu._lib.load(), gpu._lib.as_dp
    y = np.zeros(129)
    for bits in (39, 41, 0):
        assert lib.admm_op_symv_compact_bits(dp(M), 129, 129, dp(x), 0, -1, 1, dp(y), None, 0, bits) == gpu._lib.E_INVALID
    for args in ((dp(M), 129, 128, dp(x), 0, -1, 1, dp(y), None, 0), (dp(M), 129, 129, dp(x), 0, -2, 1, dp(y), None, 0),
                 (dp(M), 129, 129, dp(x), 0, -1, 0, dp(y), None, 0), (dp(M), 129, 129, dp(x), 0, -1, 1, dp(y), dp(M), 5)):
        assert lib.admm_op_symv_compact_bits(*args, 40) == gpu._lib.E_INVALID


# ===================================================================================== engine level
def _hbm_order():
    """the smallest n whose 48-bit compact store is larger than kSymvCacheBytes: read from kernels.h, not guessed"""
    txt = open(os.path.join(ROOT, "admm-project_amd", "csrc", "kernels.h")).read()
    m = re.search(r"kSymvCacheBytes\s*=\s*int64_t\{(\d+)\}\s*<<\s*(\d+)", txt)
    limit = int(m.group(1)) << int(m.group(2))
    nt = 1
    while nt * 8 * T * T + (nt * (nt + 1) // 2 - nt) * 6 * T * T <= limit:
        nt += 1
    return (nt - 1) * T + 1, nt


def _err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    if ref.ndim == 1:
        scale = np.maximum(np.abs(ref), 1e-12 + 1e-3 * np.max(np.abs(ref)))
        return float(np.max(np.abs(got - ref) / scale))
    return float(np.max(np.abs(got - ref)) / max(1e-300, np.max(np.abs(ref))))


def test_engine_adopts_the_40_bit_form_where_the_inverse_streams_from_hbm(gpu):
    """m = 2n, rho = 1 at the smallest order whose 48-bit store exceeds kSymvCacheBytes: create() builds the 40-bit
    form, its probe passes the unchanged acceptance rule, the fp64 triangle is freed; 15 iterations against the oracle
    at the suite's 1e-9."""
    from threadpoolctl import threadpool_limits

    from oracle import solvers_ref

    n, nt = _hbm_order()
    with threadpool_limits(limits=gpu.synth.host_cores()):
        p = gpu.synth.lasso_problem(seed=1, rows=2 * n, cols=n)
        opts = dict(rho=1.0, maxiters=15, domaxiters=1, objevals=1)
        got = gpu.lasso(p["D"], p["s"], p["lam"], dict(opts, xsolve="inverse"))
        ref = solvers_ref.lasso(p["D"], p["s"], p["lam"], dict(opts))
    st = got["xsolve_storage"]
    print("xsolve_storage:", st)
    assert got["engine_info"]["xsolve_used"] == "inverse"
    assert st["form"] == "compact40"
    ntri = nt * (nt + 1) // 2
    assert st["stored_bytes"] == nt * 8 * T * T + (ntri - nt) * 5 * T * T
    info = got["engine_info"]
    assert info["xsolve_cacheable_bytes"] + info["xsolve_stream_bytes"] == st["stored_bytes"]
    assert gpu._lib.load().admm_xsolve_compact_accept(st["probe_err_compact"], st["probe_err_fp64"], st["probe_diff"]) == 1
    assert np.isfinite(st["probe_err_fp64"])
    assert got["steps"] == ref["steps"] == 15
    errs = {k: _err(got[k], ref[k]) for k in ("xvals", "zvals", "uvals", "pnorm", "dnorm", "perr", "derr", "objevals")}
    print("max-norm relative errors against the oracle:", errs)
    assert all(v < 1e-9 for v in errs.values()), errs
