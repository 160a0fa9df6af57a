"""The 36- and 38-bit widths of the compact x-solve storage (csrc/tri_tile.h), host side: where the tiles lie
(admm_symv_compact_tile_offset against the byte formula), what the operator and the getters refuse before they touch a
device, and a NumPy model of the format written here -- quantise, pack into the panel records, unpack -- that the GPU
tests (test_gpu_symv_compact_narrow.py) compare the pack kernel with.

The model follows the layout, not the kernel: a tile is 32 panel records (columns 4p .. 4p + 3), a record is run 0 and
run 1 (the low dwords, 16 bytes per lane) and run 2, the lane's eight high fields of BITS - 32 bits, lowest bits first:
one dword per lane at 36 bits; at 38 bits a dword run (bits 0 .. 31) followed by a 16-bit run (bits 32 .. 47).  The
same code packs 40 and 48 bits (8 / 16 bytes per lane), which the GPU test uses to pin those two widths."""
import ctypes as C

import numpy as np
import pytest

T = 128
WIDTHS = (36, 38, 40, 48)


# ===================================================================================== the model
def quantise_tile(blk, bits):
    """(q, scale): q int64 = rint(blk / scale) clamped to +-(2^(bits-1) - 1), scale = 2^(e - (bits - 1)) with the
    tile's largest magnitude < 2^e; an all-zero tile has scale 0"""
    mx = float(np.max(np.abs(blk)))
    if mx == 0.0:
        return np.zeros(blk.shape, dtype=np.int64), 0.0
    _, e = np.frexp(mx)  # mx = f * 2^e, f in [0.5, 1)
    lim = 2.0 ** (bits - 1) - 1
    q = np.clip(np.rint(np.ldexp(blk, bits - 1 - int(e))), -lim, lim).astype(np.int64)
    return q, float(np.ldexp(1.0, int(e) - (bits - 1)))


def _hi_runs(bits):
    """run 2 as (dtype, bit offset) pieces, one piece per lane in each"""
    hb = bits - 32
    if bits == 38:
        return [(np.uint32, 0), (np.uint16, 32)]
    return [(np.uint32, 32 * k) for k in range(8 * hb // 32)]


def tile_bytes(bits):
    return bits * T * T // 8


def pack_tile(q, bits):
    """the tile's bytes (uint8 array of tile_bytes(bits)) from its T x T int64 q"""
    hb = bits - 32
    lo = (q & 0xFFFFFFFF).astype(np.uint32)
    hi = ((q >> 32) & ((1 << hb) - 1)).astype(np.uint64)  # two's complement, hb bits
    out = []
    for p in range(T // 4):
        c = 4 * p
        for run in range(2):  # lane l: (2l, c'), (2l + 1, c'), (2l, c' + 1), (2l + 1, c' + 1), c' = c + 2 run
            cc = c + 2 * run
            piece = np.stack([lo[0::2, cc], lo[1::2, cc], lo[0::2, cc + 1], lo[1::2, cc + 1]], axis=1)
            out.append(np.ascontiguousarray(piece).view(np.uint8).reshape(-1))
        h = np.zeros(T // 2, dtype=object)  # the lane's 8 hb bits as one integer
        for k in range(4):
            for par in range(2):
                f = [int(v) for v in hi[par::2, c + k]]
                h = h + np.array([v << ((2 * k + par) * hb) for v in f], dtype=object)
        for dt, off in _hi_runs(bits):
            mask = (1 << (8 * np.dtype(dt).itemsize)) - 1
            out.append(np.array([(int(v) >> off) & mask for v in h], dtype=dt).view(np.uint8).reshape(-1))
    b = np.concatenate(out)
    assert b.size == tile_bytes(bits)
    return b


def unpack_tile(b, scale, bits, sign_extend=True):
    """the T x T doubles a tile's bytes stand for: (hi * 2^32 + lo) * scale, hi sign-extended from bits - 32 bits"""
    hb = bits - 32
    rec = tile_bytes(bits) // (T // 4)
    out = np.zeros((T, T))
    for p in range(T // 4):
        r = b[p * rec:(p + 1) * rec]
        lo = np.zeros((T, 4), dtype=np.uint32)
        for run in range(2):
            piece = r[1024 * run:1024 * (run + 1)].view(np.uint32).reshape(T // 2, 4)
            lo[0::2, 2 * run], lo[1::2, 2 * run] = piece[:, 0], piece[:, 1]
            lo[0::2, 2 * run + 1], lo[1::2, 2 * run + 1] = piece[:, 2], piece[:, 3]
        h = np.zeros(T // 2, dtype=object)
        at = 2048
        for dt, off in _hi_runs(bits):
            nb = (T // 2) * np.dtype(dt).itemsize
            vals = r[at:at + nb].view(dt)
            h = h + np.array([int(v) << off for v in vals], dtype=object)
            at += nb
        assert at == rec
        for k in range(4):
            for par in range(2):
                f = np.array([(int(v) >> ((2 * k + par) * hb)) & ((1 << hb) - 1) for v in h], dtype=np.int64)
                if sign_extend:
                    f = np.where(f >= (1 << (hb - 1)), f - (1 << hb), f)
                val = f.astype(np.float64) * 4294967296.0 + lo[par::2, k].astype(np.float64)  # exact: bits <= 53
                out[par::2, 4 * p + k] = val * scale
    return out


def model_matrix(S, bits):
    """the symmetric matrix the compact storage of S's lower triangle stands for, through pack_tile / unpack_tile"""
    n = S.shape[0]
    nt = -(-n // T)
    P = np.zeros((nt * T, nt * T))
    P[:n, :n] = np.tril(S)
    Q = P.copy()
    for bi in range(nt):
        for bj in range(bi):
            blk = P[bi * T:(bi + 1) * T, bj * T:(bj + 1) * T]
            q, scale = quantise_tile(blk, bits)
            Q[bi * T:(bi + 1) * T, bj * T:(bj + 1) * T] = unpack_tile(pack_tile(q, bits), scale, bits)
    Q = Q[:n, :n]
    return np.tril(Q) + np.tril(Q, -1).T


def special_tile(kind, bits, rng):
    """a T x T tile of the kinds the format can break on"""
    blk = rng.standard_normal((T, T))
    if kind == "clamp":  # +-(2^e - scale / 4) round to +-2^(bits-1) units and are stored as +-(2^(bits-1) - 1)
        blk *= 4.0 / np.max(np.abs(blk))
        blk[-1, 77] = -8.0 * (1.0 - 2.0 ** -(bits + 1))
        blk[5, 3] = 8.0 * (1.0 - 2.0 ** -(bits + 1))
    elif kind == "zero":
        blk[:] = 0.0
    elif kind == "pow2":  # the maximum is exactly 2^-3: e = -2, one binade above the exponent of the other entries
        blk *= 0.1 / np.max(np.abs(blk))
        blk[0, 5] = 0.125
    else:
        assert kind == "plain"
    return blk


# ===================================================================================== tests
@pytest.mark.parametrize("kind", ["plain", "clamp", "zero", "pow2"])
@pytest.mark.parametrize("bits", [36, 38])
def test_model_quantise_pack_unpack(bits, kind):
    """unpack(pack(q)) is q * scale bit for bit; the clamp acts at both ends; an all-zero tile stays zero with scale 0;
    a power-of-two maximum gets the binade above it.  Reading the high field without its sign (the mistake that broke
    19 of 20 cases of the 40-bit form) changes every tile that holds a negative entry."""
    rng = np.random.default_rng(100 * bits + len(kind))
    blk = special_tile(kind, bits, rng)
    q, scale = quantise_tile(blk, bits)
    b = pack_tile(q, bits)
    assert b.size == bits * T * T // 8 == {36: 72, 38: 76}[bits] * 1024
    back = unpack_tile(b, scale, bits)
    want = q.astype(np.float64) * scale  # exact: |q| < 2^53, scale a power of two
    assert np.array_equal(back.view(np.uint64), want.view(np.uint64))
    lim = 2 ** (bits - 1) - 1
    assert np.max(np.abs(q)) <= lim
    if kind == "clamp":
        assert q[-1, 77] == -lim and q[5, 3] == lim and scale == 2.0 ** (4 - bits)
        assert blk[-1, 77] < back[-1, 77] and blk[5, 3] > back[5, 3]  # a whole unit off, towards zero
    elif kind == "zero":
        assert scale == 0.0 and not b.any() and not back.any()
    elif kind == "pow2":
        assert scale == 2.0 ** (-2 - (bits - 1)) and back[0, 5] == 0.125 and q[0, 5] == 2 ** (bits - 2)
    else:
        assert np.max(np.abs(back - blk)) <= scale / 2
    if kind != "zero":
        assert (q < 0).any()
        wrong = unpack_tile(b, scale, bits, sign_extend=False)
        assert np.array_equal(wrong[q >= 0], back[q >= 0]) and np.all(wrong[q < 0] != back[q < 0])


def _offset(lib, L, n, bits, t):
    off = C.c_int64(-1)
    L.check(lib.admm_symv_compact_tile_offset(n, bits, t, C.byref(off)))
    return off.value


@pytest.mark.parametrize("bits", WIDTHS)
def test_tile_offsets_and_stored_bytes_follow_the_formula(ap, bits):
    """tile t starts after the tiles before it, a diagonal tile 8 T^2 bytes and an off-diagonal one BITS / 8 T^2; the
    store is nt 8 T^2 + (nt (nt + 1) / 2 - nt) BITS / 8 T^2 bytes; every tile starts on a multiple of 4 KB, so that
    every lane load (16, 4 and 2 bytes at multiples of their size inside a 128-byte-aligned record) is aligned"""
    L = ap._lib
    lib = L.load()
    assert (tile_bytes(bits) // 32) % 128 == 0  # the panel record
    for n in (1, 128, 129, 300, 513, 8193, 10000):
        nt = -(-n // T)
        ntri = nt * (nt + 1) // 2
        want, t = 0, 0
        for bi in range(nt if nt <= 6 else 3):
            for bj in range(bi + 1):
                got = _offset(lib, L, n, bits, t)
                assert got == want and got % 4096 == 0, (n, bits, t, got, want)
                want += 8 * T * T if bi == bj else tile_bytes(bits)
                t += 1
        total = _offset(lib, L, n, bits, ntri)
        assert total == nt * 8 * T * T + (ntri - nt) * bits * T * T // 8, (n, bits)
        last = _offset(lib, L, n, bits, ntri - 1)  # the last tile is diagonal
        assert total - last == 8 * T * T and last % 4096 == 0
    assert tile_bytes(36) == 72 * 1024 and tile_bytes(38) == 76 * 1024


def test_headline_store_sizes(ap):
    """n = 10^4: 79 diagonal tiles of 128 KB and 3081 off-diagonal ones"""
    L = ap._lib
    lib = L.load()
    nt, ntri = 79, 3160
    for bits, mb in ((36, 237.5), (38, 250.1), (40, 262.8)):
        total = _offset(lib, L, 10000, bits, ntri)
        assert total == nt * 131072 + (ntri - nt) * bits * 2048
        assert abs(total * 1e-6 - mb) < 0.06, (bits, total)


def test_refusals_before_touching_a_device(ap):
    L = ap._lib
    lib, dp = L.load(), L.as_dp
    M, x, y = np.eye(4, order="F"), np.ones(4), np.zeros(4)
    for bits in (36, 38):
        assert lib.admm_op_symv_compact_bits(None, 4, 4, dp(x), 0, -1, 1, dp(y), None, 0, bits) == L.E_INVALID
        assert lib.admm_op_symv_compact_bits(dp(M), 4, 4, None, 0, -1, 1, dp(y), None, 0, bits) == L.E_INVALID
        assert lib.admm_op_symv_compact_bits(dp(M), 4, 4, dp(x), 0, -1, 1, None, None, 0, bits) == L.E_INVALID
        assert lib.admm_op_symv_compact_bits(dp(M), 0, 4, dp(x), 0, -1, 1, dp(y), None, 0, bits) == L.E_INVALID
        assert lib.admm_op_symv_compact_bits(dp(M), 4, 3, dp(x), 0, -1, 1, dp(y), None, 0, bits) == L.E_INVALID
        assert lib.admm_op_symv_compact_bits(dp(M), 4, 4, dp(x), 0, -2, 1, dp(y), None, 0, bits) == L.E_INVALID
        assert lib.admm_op_symv_compact_bits(dp(M), 4, 4, dp(x), 0, -1, 0, dp(y), None, 0, bits) == L.E_INVALID
        assert lib.admm_op_symv_compact_bits(dp(M), 4, 4, dp(x), 0, -1, 1, dp(y), dp(M), 3, bits) == L.E_INVALID
    for bits in (35, 37, 39, 34, 33, 32, -36, -38):
        assert lib.admm_op_symv_compact_bits(dp(M), 4, 4, dp(x), 0, -1, 1, dp(y), None, 0, bits) == L.E_INVALID
    off = C.c_int64(0)
    for bits in (0, 35, 37, 39, 41, 64):
        assert lib.admm_symv_compact_tile_offset(300, bits, 0, C.byref(off)) == L.E_INVALID
    for n, t in ((0, 0), (300, -1), (300, 7)):  # 300: 3 tile rows, 6 tiles
        assert lib.admm_symv_compact_tile_offset(n, 36, t, C.byref(off)) == L.E_INVALID
    assert lib.admm_symv_compact_tile_offset(300, 36, 0, None) == L.E_INVALID
    cnt = C.c_int32(0)
    assert lib.admm_engine_xsolve_rejected(None, 0, C.byref(cnt), None, None, None, None) == L.E_INVALID
    assert (L.STORAGE_FP64, L.STORAGE_COMPACT, L.STORAGE_COMPACT40, L.STORAGE_COMPACT38, L.STORAGE_COMPACT36) == \
        (0, 1, 2, 3, 4)
