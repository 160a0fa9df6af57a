"""The 36- and 38-bit widths of the compact x-solve storage (csrc/tri_tile.h) on the device, through
admm_op_symv_compact_bits (pack kernel + compact product) against the NumPy model of test_symv_compact_narrow_host.py,
which packs every off-diagonal tile into the bytes of the layout and reads them back; and once through the engine,
which tries 36 and 38 bits before 40 where even the 40-bit store is larger than kSymvCacheBytes.

No measured tolerance, as in test_gpu_symv_compact40.py: the dequantised matrix is compared bit for bit, the product
with the summation bound (n + 4) * 2^-53 * |Q||x| against a longdouble reference.

Fault injection (each on a scratch copy of the sources, never committed): see EXPERIMENTS.md, "36- and 38-bit compact
tiles", for which assertion of this file caught the high field read without its sign and the scale exponent off by
one, at either width."""
import functools
import os
import re

import numpy as np
import pytest

from test_symv_compact_narrow_host import T, model_matrix

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("plain", "pow2", "zero", "span32", "negmax")
ORDERS = (128, 129, 300, 513)  # one tile and no off-diagonal one; ragged last tiles; three and five tile rows


@functools.lru_cache(maxsize=None)
def _case(n, kind, bits):
    """(S, x, Q, refQ, boundQ): S symmetric with a dominant diagonal; `kind` reshapes the LAST off-diagonal tile of the
    first tile column (at n = 129 and 513 one live row and 127 rows of padding; none at n = 128, where S stays plain)"""
    rng = np.random.default_rng(9000 * n + 10 * KINDS.index(kind) + bits)
    low = np.tril(rng.standard_normal((n, n)))
    low[np.diag_indices(n)] += 300.0 * (1.0 + rng.random(n))  # hundreds of times the rest of its tile
    nt = -(-n // T)
    r0 = (nt - 1) * T
    if nt > 1:
        blk = low[r0:, :T]  # a view: tile (nt - 1, 0)
        if kind == "pow2":  # the tile's maximum is exactly 2^-3: e = -2
            blk *= 0.1 / np.max(np.abs(blk))
            blk[0, 5] = 0.125
        elif kind == "zero":
            blk[:] = 0.0
        elif kind == "span32":  # magnitudes 2^-32 .. 1 under a maximum of 1.5: the grid is 2^(2 - bits)
            blk *= np.ldexp(1.0 / np.max(np.abs(blk)), -rng.integers(0, 33, blk.shape))
            blk[0, 0], blk[-1, -1] = 1.5, 1.5 * 2.0 ** -bits  # (the last one is 3/8 of a unit: stored as 0)
        elif kind == "negmax":  # +-2^(bits-1) units after rounding: clamped to +-(2^(bits-1) - 1)
            blk *= 4.0 / np.max(np.abs(blk))
            blk[-1, 77] = -8.0 * (1.0 - 2.0 ** -(bits + 1))
            blk[-1, 78] = 8.0 * (1.0 - 2.0 ** -(bits + 1))
    S = low + np.tril(low, -1).T
    x = rng.standard_normal(n)
    Q = model_matrix(S, bits)
    xl = x.astype(LD)
    refQ = Q.astype(LD) @ xl
    boundQ = (n + 4) * LD(U) * (np.abs(Q).astype(LD) @ np.abs(xl))
    for a in (S, x, Q, refQ, boundQ):
        a.setflags(write=False)
    return S, x, Q, refQ, boundQ


def _lower_storage(S):
    M = np.asfortranarray(S.copy())
    M[np.triu_indices(S.shape[0], 1)] = np.nan  # the kernels read the lower triangle only
    return M


def _op(gpu, M, n, x, fin, ncached, parts, bits, want_q=False):
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
    """properties of the inputs themselves (model only), at both widths"""
    n, r0 = 300, 256
    for bits in (36, 38):
        lim = 2.0 ** (bits - 1) - 1
        S, _, Q, *_ = _case(n, "negmax", bits)
        assert Q[r0 + 43, 77] == -lim * 2.0 ** (4 - bits) and S[r0 + 43, 77] < Q[r0 + 43, 77]
        assert Q[r0 + 43, 78] == lim * 2.0 ** (4 - bits) and S[r0 + 43, 78] > Q[r0 + 43, 78]
        S, _, Q, *_ = _case(n, "span32", bits)
        blkS, blkQ = S[r0:, :T], Q[r0:, :T]
        assert blkQ[-1, -1] == 0.0 and np.count_nonzero((blkQ == 0.0) & (blkS != 0.0)) >= 1
        assert np.max(np.abs(blkS)) == 1.5
        S, _, Q, *_ = _case(n, "pow2", bits)
        assert np.max(np.abs(S[r0:, :T])) == 0.125 and Q[r0, 5] == 0.125
        S, _, Q, *_ = _case(n, "plain", bits)
        assert (Q[r0:, :T] < 0).any() and not np.array_equal(Q, S)  # negative high fields; the format does round


@pytest.mark.parametrize("n,kind", [(n, k) for n in ORDERS for k in KINDS if n > T or k == "plain"])  # (one tile: plain)
@pytest.mark.parametrize("bits", [36, 38])
def test_narrow_product_against_the_model(gpu, bits, n, kind):
    """The matrix the kernel multiplied is the model's bit for bit (pack kernel: exponent, rounding, clamp, the hi / lo
    split, the layout as the product kernel reads it back); y = Q x inside the summation bound, the same bits for
    every cache split and with or without the finalize passenger; three dealt parts add up inside the same bound."""
    S, x, Q, refQ, boundQ = _case(n, kind, bits)
    M = _lower_storage(S)
    y0, Qg = _op(gpu, M, n, x, 0, -1, 1, bits, want_q=True)
    assert np.array_equal(Qg.view(np.uint64), np.asfortranarray(Q).view(np.uint64)), "dequantised matrix differs"
    if kind == "zero":
        assert not Qg[(-(-n // T) - 1) * T:, :T].any()
    worst = 0.0
    for fin in (0, 1):
        for nc in (0, _tiles(n), -1):
            for parts in (1, 3):
                y = _op(gpu, M, n, x, fin, nc, parts, bits)
                assert not np.isnan(y).any(), (fin, nc, parts)
                eq = np.abs(y.astype(LD) - refQ)
                worst = max(worst, float(np.max(eq / boundQ)))
                assert np.all(eq <= boundQ), (fin, nc, parts, float(np.max(eq / boundQ)))
                if parts == 1:
                    assert np.array_equal(y.view(np.uint64), y0.view(np.uint64)), (fin, nc)
    print(f"symv_compact{bits} n={n} {kind}: worst |y - Qx| / bound = {worst:.3f}")


@pytest.mark.parametrize("n", [129, 513])
def test_40_and_48_bits_are_what_they_were(gpu, n):
    """48 bits through the width-selecting entry is admm_op_symv_compact bit for bit; 40 bits packs to the model's
    matrix (the same byte model at that width) and multiplies inside the summation bound"""
    S, x, *_ = _case(n, "negmax", 40)
    M = _lower_storage(S)
    lib, dp = gpu._lib.load(), gpu._lib.as_dp
    for fin, parts in ((0, 1), (1, 1), (0, 3)):
        y_old, Q_old = np.full(n, np.nan), np.full((n, n), np.nan, order="F")
        gpu._lib.check(lib.admm_op_symv_compact(dp(M), n, n, dp(x), fin, -1, parts, dp(y_old), dp(Q_old), n))
        y_new, Q_new = _op(gpu, M, n, x, fin, -1, parts, 48, want_q=True)
        assert not np.isnan(y_new).any() and not np.isnan(Q_new).any()
        assert np.array_equal(y_new.view(np.uint64), y_old.view(np.uint64)), (fin, parts)
        assert np.array_equal(Q_new.view(np.uint64), Q_old.view(np.uint64)), (fin, parts)
    assert np.array_equal(Q_old.view(np.uint64), np.asfortranarray(model_matrix(S, 48)).view(np.uint64))
    S, x, Q, refQ, boundQ = _case(n, "negmax", 40)
    for fin in (0, 1):
        y, Qg = _op(gpu, M, n, x, fin, -1, 1, 40, want_q=True)
        assert np.array_equal(Qg.view(np.uint64), np.asfortranarray(Q).view(np.uint64))
        assert np.all(np.abs(y.astype(LD) - refQ) <= boundQ)


def test_other_widths_are_refused(gpu):
    S, x, *_ = _case(129, "plain", 36)
    M = _lower_storage(S)
    lib, dp = gpu._lib.load(), gpu._lib.as_dp
    y = np.zeros(129)
    for bits in (35, 37, 39, 0):
        assert lib.admm_op_symv_compact_bits(dp(M), 129, 129, dp(x), 0, -1, 1, dp(y), None, 0, bits) == gpu._lib.E_INVALID


# ===================================================================================== engine level
def _cache_limit():
    txt = open(os.path.join(ROOT, "admm-project_amd", "csrc", "kernels.h")).read()
    m = re.search(r"kSymvCacheBytes\s*=\s*int64_t\{(\d+)\}\s*<<\s*(\d+)", txt)
    return int(m.group(1)) << int(m.group(2))


def _stored(nt, bits):
    return nt * 8 * T * T + (nt * (nt + 1) // 2 - nt) * bits * T * T // 8


def _narrow_order():
    """the smallest n whose 40-bit compact store is larger than kSymvCacheBytes: read from kernels.h, not guessed"""
    limit = _cache_limit()
    nt = 1
    while _stored(nt, 40) <= limit:
        nt += 1
    return (nt - 1) * T + 1, nt


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref)) / max(1e-300, np.max(np.abs(ref))))


def test_engine_ladder_where_the_40_bit_store_streams_from_hbm(gpu):
    """m = 2n, rho = 1 at the smallest order whose 40-bit store exceeds kSymvCacheBytes: create() tries 36 and 38 bits
    before 40; the form kept passes the unchanged acceptance rule and every rung reported as rejected fails it; the
    bytes are the kept form's formula; 15 forced iterations agree with the same loop over the fp64 inverse (the engine
    LassoMulti builds keeps fp64 storage) within the suite's 1e-9.
    Measured on MI355X at n = 8193: 36 bits probes at 6.5e-11 / 2.8e-11 and 38 bits at 1.7e-11 / 7.1e-12 (err / diff,
    against the floor of 1e-11), both rejected; 40 bits at 4.0e-12 / 2.1e-12 is kept."""
    from threadpoolctl import threadpool_limits

    n, nt = _narrow_order()
    assert _stored(nt - 1, 40) <= _cache_limit() < _stored(nt, 40)
    lib = gpu._lib.load()
    with threadpool_limits(limits=gpu.synth.host_cores()):
        p = gpu.synth.lasso_problem(seed=1, rows=2 * n, cols=n)
        opts = dict(rho=1.0, maxiters=15, domaxiters=1)
        got = gpu.lasso(p["D"], p["s"], p["lam"], dict(opts, xsolve="inverse"))
        multi = gpu.LassoMulti(p["D"], p["s"], [p["lam"]], rho=1.0, xsolve="inverse")
        try:
            ref = multi.results(multi.run(maxiters=15, domaxiters=1))
        finally:
            multi.close()
    st = got["xsolve_storage"]
    print("xsolve_storage:", st)
    assert got["engine_info"]["xsolve_used"] == "inverse" and ref["xsolve"] == "inverse"
    assert st["form"] in ("compact36", "compact38", "compact40")
    kept = int(st["form"][len("compact"):])
    assert st["stored_bytes"] == _stored(nt, kept)
    info = got["engine_info"]
    assert info["xsolve_cacheable_bytes"] + info["xsolve_stream_bytes"] == st["stored_bytes"]
    assert lib.admm_xsolve_compact_accept(st["probe_err_compact"], st["probe_err_fp64"], st["probe_diff"]) == 1
    assert np.isfinite(st["probe_err_fp64"])
    assert [r["bits"] for r in st["rejected"]] == [b for b in (36, 38, 40) if b < kept]  # the order tried
    for r in st["rejected"]:
        assert lib.admm_xsolve_compact_accept(r["probe_err_compact"], r["probe_err_fp64"], r["probe_diff"]) == 0, r
    assert got["steps"] == 15 and int(ref["steps"][0]) == 15
    errs = {k: _rel(got[k], ref[k]) for k in ("xopt", "zopt", "uopt", "pnorm", "dnorm", "perr", "derr")}
    print("max-norm relative differences against the fp64-storage engine:", errs)
    assert all(v < 1e-9 for v in errs.values()), errs
