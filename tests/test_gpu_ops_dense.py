"""The symmetric lower-triangle product (symv.hip) and the dense setup kernels (dense.hip: MFMA GEMM, factor inverse,
L*(L'*x)) through their operator entry points, each against a plain reference at the sizes where a tile kernel goes
wrong: one tile, a multiple of 128, one past it, one short of it, odd orders, several tiles.

Two kinds of reference, no measured tolerance anywhere:

exact    integer data, |value| <= 2^20 and inner length <= 700: every product and every partial sum is an integer
         below 2^53, so the fp64 result is the same in ANY summation order, with or without FMA.  The reference is
         NumPy int64 arithmetic; the assertion is array_equal.  A dropped, doubled or misrouted element, or an fp32
         intermediate, has nowhere to hide.
bounded  standard-normal data against an np.longdouble reference, element-wise
             |got - ref| <= (k + 4) * 2^-53 * (|alpha| |A||B| + |beta| |C|)          (symv: |M||x|)
         with k the length of the inner sum: the recursive-summation bound (Higham, Accuracy and Stability, 3.1),
         which holds for every order of the additions and for fused or unfused multiply-adds; + 4 covers the
         roundings of alpha, beta and the final addition.  NumPy's own fp64 product of the same inputs is asserted to
         sit inside the bound next to every kernel result, so the bound is never tighter than fp64 allows.

Each test prints the worst |error| / bound it saw (pytest -s shows them; EXPERIMENTS.md records a run).
"""
import functools

import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
IMAX = 2 ** 20
SENTINEL = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]  # a NaN with a payload of its own


def _dp(ap, a):
    return ap._lib.as_dp(a)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (the assertion is ratio <= 1); a zero bound admits a zero error only"""
    err = np.abs(got.astype(LD) - ref)
    if np.any(np.isnan(err)):
        return np.inf
    safe = np.where(bound > 0, bound, LD(1))
    return float(np.max(np.where(bound > 0, err / safe, np.where(err == 0, LD(0), LD(np.inf)))))


def _store(a, ld, fill=np.nan):
    """a as the top rows of an ld-row column-major buffer; the padding rows hold `fill` (NaN: reading one poisons)"""
    buf = np.full((ld, a.shape[1]), fill, order="F")
    buf[:a.shape[0]] = a
    return buf


# ===================================================================================== symmetric product
SYMV_ORDERS = [1, 2, 127, 128, 129, 255, 256, 257, 383, 385, 641]


def _tiles(n):
    t = -(-n // 128)
    return t * (t + 1) // 2


def _ncached_values(n):
    return sorted({-1, 0, 1, _tiles(n) - 1, _tiles(n)})


@functools.lru_cache(maxsize=None)
def _symv_case(n, kind, seed=0):
    """(S, x, ref, bound): S full symmetric; kind 'int' -> ref exact (bound None), 'normal' -> longdouble ref + bound"""
    rng = np.random.default_rng(1000 * n + seed + (7 if kind == "int" else 0))
    if kind == "int":
        low = np.tril(rng.integers(-IMAX, IMAX + 1, (n, n)))
        S = low + np.tril(low, -1).T
        x = rng.integers(-IMAX, IMAX + 1, n)
        ref = (S @ x).astype(np.float64)  # int64 arithmetic: |sum| <= 641 * 2^40 < 2^53
        assert np.max(np.abs(S).astype(np.int64) @ np.abs(x)) < 2 ** 53
        return S.astype(np.float64), x.astype(np.float64), ref, None
    low = np.tril(rng.standard_normal((n, n)))
    S = low + np.tril(low, -1).T
    x = rng.standard_normal(n)
    ref = S.astype(LD) @ x.astype(LD)
    bound = (n + 4) * LD(U) * (np.abs(S).astype(LD) @ np.abs(x).astype(LD))
    assert _ratio(S @ x, ref, bound) <= 1.0  # NumPy's fp64 product obeys the bound
    return S, x, ref, bound


def _lower_storage(S, ld=None):
    """the kernels' contract (kernels.h: "from its lower triangle only"): NaN strictly above the diagonal"""
    n = S.shape[0]
    M = S.copy()
    M[np.triu_indices(n, 1)] = np.nan
    return _store(M, n if ld is None else ld)


def _full_storage(S):
    n = S.shape[0]
    return _store(S, n + (n & 1))  # the small form wants an even leading dimension


def _symv(gpu, M, n, x, form, ncached=-1, parts=1):
    y = np.full(n, np.nan)
    gpu._lib.check(gpu._lib.load().admm_op_symv(_dp(gpu, M), n, M.shape[0], _dp(gpu, x), form, ncached, parts,
                                                _dp(gpu, y)))
    return y


def _symv_batch(gpu, mats, n, X, ncached=-1):
    K = len(mats)
    Ms = np.asfortranarray(np.concatenate(mats, axis=1))  # back to back, ldM = n
    Xf = np.asfortranarray(X)
    Y = np.full((n, K), np.nan, order="F")
    gpu._lib.check(gpu._lib.load().admm_op_symv_batch(_dp(gpu, Ms), n, n, K, _dp(gpu, Xf), n, ncached, _dp(gpu, Y), n))
    return Y


@pytest.mark.parametrize("n", SYMV_ORDERS)
def test_symv_exact(gpu, n):
    """Every form, every cache split, integer data: bitwise the int64 product.  Forms 1 - 3 get NaN above the diagonal.
    Catches `(s.r > j)` -> `(s.r >= j)` in sy_compute (the diagonal would be counted in both the N- and the T-part:
    wrong at every order here, 1 and 2 included), a wrong lane of reduce_scatter4, a clamp that reads x past n at the
    odd orders, a live row lost in the last tile (129, 257, 385, 641)."""
    S, x, ref, _ = _symv_case(n, "int")
    np.testing.assert_array_equal(_symv(gpu, _full_storage(S), n, x, 0), ref)
    M = _lower_storage(S)
    for form in (1, 2, 3):
        for nc in _ncached_values(n):
            np.testing.assert_array_equal(_symv(gpu, M, n, x, form, nc), ref, err_msg=f"form {form} ncached {nc}")


@pytest.mark.parametrize("n", SYMV_ORDERS)
def test_symv_bounded(gpu, n):
    """Normal data inside the summation bound; the load flavour (default / non-temporal, any split) does not change
    the arithmetic, so all cache splits of one form give the same bits; forms 2 and 3 run the same symv_lower_body<true>
    and the same reduction, so they agree bitwise; a second call repeats the first bit for bit (fixed-order sums)."""
    S, x, ref, bound = _symv_case(n, "normal")
    worst = _ratio(_symv(gpu, _full_storage(S), n, x, 0), ref, bound)
    M = _lower_storage(S)
    first = {}
    for form in (1, 2, 3):
        for nc in _ncached_values(n):
            y = _symv(gpu, M, n, x, form, nc)
            worst = max(worst, _ratio(y, ref, bound))
            assert _same_bits(y, first.setdefault(form, y)), f"form {form}: ncached {nc} changed the bits"
        assert _same_bits(_symv(gpu, M, n, x, form), first[form]), f"form {form}: not reproducible"
    assert _same_bits(first[2], first[3])
    y0 = _symv(gpu, _full_storage(S), n, x, 0)
    assert _same_bits(y0, _symv(gpu, _full_storage(S), n, x, 0))
    print(f"symv n={n}: worst |err|/bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("n,ld", [(5, 6), (5, 8), (6, 6), (6, 10), (129, 130), (130, 132), (641, 644)])
def test_symv_small_leading_dimension(gpu, n, ld):
    """the small form (one wave per column, 16-byte pairs + the odd tail element) with odd and even n, ld > n"""
    S, x, ref, _ = _symv_case(n, "int", seed=3)
    np.testing.assert_array_equal(_symv(gpu, _store(S, ld), n, x, 0), ref)
    S, x, ref, bound = _symv_case(n, "normal", seed=3)
    assert _ratio(_symv(gpu, _store(S, ld), n, x, 0), ref, bound) <= 1.0


@pytest.mark.parametrize("n", [129, 385, 641])
@pytest.mark.parametrize("parts", [2, 3, 7])
def test_symv_tile_deal(gpu, n, parts):
    """part_rank / part_count: rank r takes the lower-triangle tiles with linear index = r (mod P), the P partial
    results add up to the product -- bitwise on integer data.  P = 7 exceeds the 3 tiles of n = 129 (ranks that own
    nothing return zeros).  What these cases catch: a tile taken by two ranks or by none (the exact sum breaks), at
    one tile row (129), three (385) and five (641, 15 tiles).  What they do NOT catch: `lin % part_count` ->
    `bi % part_count` -- that deal is unbalanced but still hands every tile to exactly one rank, and the operator
    returns only the sum of the ranks' results, so this mutation passes."""
    S, x, ref, _ = _symv_case(n, "int")
    M = _lower_storage(S)
    for form in (1, 2, 3):
        np.testing.assert_array_equal(_symv(gpu, M, n, x, form, -1, parts), ref, err_msg=f"form {form}")
    S, x, ref, bound = _symv_case(n, "normal")
    M = _lower_storage(S)
    for form in (1, 2, 3):
        y = _symv(gpu, M, n, x, form, 1, parts)
        assert _ratio(y, ref, bound) <= 1.0
        assert _same_bits(y, _symv(gpu, M, n, x, form, 1, parts))


@pytest.mark.parametrize("n", [129, 257])
def test_symv_batch_matches_single_launches(gpu, n):
    """K = 3 different matrices and vectors in one batched launch: every slice is bitwise what forms 2 and 3 give for
    that matrix alone (same body, same reduction order), exact on integers and inside the bound on normal data;
    catches a slice stride or a pointer-table mix-up (slice k reading matrix or vector k')"""
    for kind in ("int", "normal"):
        cases = [_symv_case(n, kind, seed=10 + k) for k in range(3)]
        mats = [_lower_storage(c[0]) for c in cases]
        X = np.stack([c[1] for c in cases], axis=1)
        for nc in (-1, 0, 1):
            Y = _symv_batch(gpu, mats, n, X, nc)
            for k, (S, x, ref, bound) in enumerate(cases):
                if kind == "int":
                    np.testing.assert_array_equal(Y[:, k], ref)
                else:
                    assert _ratio(Y[:, k], ref, bound) <= 1.0
                assert _same_bits(Y[:, k], _symv(gpu, mats[k], n, x, 2, nc))
                assert _same_bits(Y[:, k], _symv(gpu, mats[k], n, x, 3, nc))
        assert _same_bits(Y, _symv_batch(gpu, mats, n, X, 1))


@pytest.mark.parametrize("k", [0, 1, 63, 64, 127, 128, 129, 255, 256])
def test_symv_unit_vector_probe(gpu, k):
    """M[r, j] = 1024 r + j (r >= j), x = e_k: y is column k of the symmetrised M, so a wrong lane, row pair or tile
    shows as the index it was taken from"""
    n = 257
    r, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    S = np.where(r >= j, 1024 * r + j, 1024 * j + r).astype(np.float64)
    x = np.zeros(n)
    x[k] = 1.0
    np.testing.assert_array_equal(_symv(gpu, _full_storage(S), n, x, 0), S[:, k])
    M = _lower_storage(S)
    for form in (1, 2, 3):
        np.testing.assert_array_equal(_symv(gpu, M, n, x, form), S[:, k], err_msg=f"form {form}")


# ===================================================================================== GEMM
GEMM_SHAPES = [(1, 1), (127, 129), (128, 128), (129, 127), (200, 257), (257, 64)]
GEMM_KS = [1, 4, 15, 16, 17, 32, 33, 100]
GEMM_AB = [(1.0, 0.0), (-1.0, 1.0), (2.0, -0.5), (0.0, 1.0)]
LD_NAMES = ("even", "odd", "padded")


def _ld(rows, cfg):
    """0: the smallest even ld >= rows, 1: the smallest odd one, 2: rows + 3"""
    return (rows + (rows & 1), rows + 1 - (rows & 1), rows + 3)[cfg]


def _gemm(gpu, ta, tb, alpha, A, B, beta, C, M, N, K, cfg, lower=0):
    """A, B as stored (before op), C the M x N input (NaN where beta == 0).  Returns the M x N result after checking
    that the rows M .. ldc-1 kept the sentinel's bits."""
    Ab, Bb = _store(A, _ld(A.shape[0], cfg)), _store(B, _ld(B.shape[0], cfg))
    ldc = _ld(M, cfg)
    Cb = _store(C, ldc, SENTINEL)
    gpu._lib.check(gpu._lib.load().admm_op_gemm(ta, tb, M, N, K, alpha, _dp(gpu, Ab), Ab.shape[0], _dp(gpu, Bb),
                                                Bb.shape[0], beta, _dp(gpu, Cb), ldc, lower))
    if ldc > M:
        assert np.all(_bits(Cb[M:]) == _bits(np.array([SENTINEL]))[0]), "rows past M of C were written"
    return Cb[:M].copy()


def _gemm_inputs(rng, ta, tb, M, N, K, kind):
    sa, sb = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
    if kind == "int":
        return (rng.integers(-IMAX, IMAX + 1, s) for s in (sa, sb, (M, N)))
    return (rng.standard_normal(s) for s in (sa, sb, (M, N)))


def _gemm_check(gpu, ta, tb, M, N, K, alpha, beta, cfg, seed, lower=0):
    """one shape, exact then bounded; returns the worst ratio of the bounded run"""
    tag = f"{'NT'[ta]}{'NT'[tb]} {M}x{N}x{K} alpha={alpha} beta={beta} ld={LD_NAMES[cfg]} lower={lower}"
    rng = np.random.default_rng(seed)
    keep = np.tril(np.ones((M, N), dtype=bool)) if lower else np.ones((M, N), dtype=bool)
    # exact
    A, B, C = _gemm_inputs(rng, ta, tb, M, N, K, "int")
    P = (A.T if ta else A) @ (B.T if tb else B)  # int64, |.| <= 100 * 2^40
    ref = (int(2 * alpha) * P + int(2 * beta) * C).astype(np.float64) / 2.0  # 2*alpha, 2*beta are integers
    Cin = C.astype(np.float64) if beta != 0.0 else np.full((M, N), np.nan)  # beta == 0 never reads C
    got = _gemm(gpu, ta, tb, alpha, A.astype(np.float64), B.astype(np.float64), beta, Cin, M, N, K, cfg, lower)
    assert np.array_equal(got[keep], ref[keep]), tag
    # bounded
    A, B, C = _gemm_inputs(rng, ta, tb, M, N, K, "normal")
    oa, ob = (A.T if ta else A).astype(LD), (B.T if tb else B).astype(LD)
    ref = LD(alpha) * (oa @ ob) + LD(beta) * C.astype(LD)
    bound = (K + 4) * LD(U) * (abs(alpha) * (np.abs(oa) @ np.abs(ob)) + abs(beta) * np.abs(C).astype(LD))
    numpy64 = alpha * ((A.T if ta else A) @ (B.T if tb else B)) + beta * C
    assert _ratio(numpy64[keep], ref[keep], bound[keep]) <= 1.0, tag  # NumPy's fp64 product obeys the bound
    Cin = C if beta != 0.0 else np.full((M, N), np.nan)
    got = _gemm(gpu, ta, tb, alpha, A, B, beta, Cin, M, N, K, cfg, lower)
    assert np.all(np.isfinite(got[keep])), tag
    ratio = _ratio(got[keep], ref[keep], bound[keep])
    assert ratio <= 1.0, (tag, ratio)
    return ratio


@pytest.mark.parametrize("si", range(len(GEMM_SHAPES)), ids=[f"{m}x{n}" for m, n in GEMM_SHAPES])
@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["NN", "TN", "NT", "TT"])
def test_gemm(gpu, ta, tb, si):
    """Every transpose pair x every (M, N) x every K; (alpha, beta) and the leading-dimension rule (smallest even,
    smallest odd, rows + 3; applied to A, B and C alike) rotate so that each pair meets every value of both.  With
    beta == 0 C arrives as NaN and must come back finite; the rows of C past M keep their sentinel.
    Catches a wrong transpose loader, beta applied where it is 0, a store past M, and a dropped k guard of the
    k-major loader (`gk + 1 < kvalid`, odd K) in these cases: TN everywhere (both operands are k-major, both take the
    stray element, their product is added); NN and TT where ld > K, so that the stray element is NaN padding (only
    one operand is k-major there, the other one's k row is guarded to 0, and a FINITE stray -- ld == K -- times 0
    vanishes); NT has no such guard (both operands t-major, the whole k row is guarded at once).  That mutation was
    reasoned, not run: it reads past the operand buffer.  NOT observable from C, here or anywhere: the t guard `gt + 1 < tvalid` -- the element it lets in
    sits in row M of the operand tile and feeds only row M of C, whose store the epilogue drops."""
    M, N = GEMM_SHAPES[si]
    pair = 2 * tb + ta
    worst = 0.0
    for ki, K in enumerate(GEMM_KS):
        alpha, beta = GEMM_AB[(ki + si + pair) % 4]
        cfg = (ki + 2 * si + pair) % 3
        worst = max(worst, _gemm_check(gpu, ta, tb, M, N, K, alpha, beta, cfg, seed=1000 * si + 10 * ki + pair))
    print(f"gemm {'NT'[ta]}{'NT'[tb]} {M}x{N}: worst |err|/bound = {worst:.3f}")


# the rotation of test_gemm gives every transpose pair every (alpha, beta) and every leading-dimension rule with every
# K at least once: checked when the module is collected (bookkeeping, no device work)
for _pair in range(4):
    _ab = {((ki + si + _pair) % 4, ki) for si in range(len(GEMM_SHAPES)) for ki in range(len(GEMM_KS))}
    _ldr = {((ki + 2 * si + _pair) % 3, ki) for si in range(len(GEMM_SHAPES)) for ki in range(len(GEMM_KS))}
    assert len(_ab) == 4 * len(GEMM_KS) and len(_ldr) == 3 * len(GEMM_KS)


@pytest.mark.parametrize("n", [1, 128, 129, 257])
@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["NN", "TN", "NT", "TT"])
def test_gemm_lower_only(gpu, ta, tb, n):
    """lower_only on square results: the lower triangle with its diagonal is asserted, the strict upper part is free
    (n = 257: the tile strictly above the diagonal is skipped as a whole, the diagonal tiles are masked per element)"""
    pair = 2 * tb + ta
    for ki, K in enumerate((17, 32)):
        alpha, beta = GEMM_AB[(ki + pair) % 4]
        _gemm_check(gpu, ta, tb, n, n, K, alpha, beta, (ki + pair) % 3, seed=77 * n + ki + pair, lower=1)


@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["NN", "TN", "NT", "TT"])
def test_gemm_fast_and_guarded_loader_agree(gpu, ta, tb):
    """128 x 128 x 32 with even leading dimensions is an interior, aligned tile: the unguarded loader.  The same
    numbers behind odd leading dimensions take the guarded one and must give the same bits."""
    rng = np.random.default_rng(5 + 2 * tb + ta)
    A, B, C = _gemm_inputs(rng, ta, tb, 128, 128, 32, "normal")
    for alpha, beta in ((1.0, 0.0), (-1.0, 1.0)):
        Cin = C if beta != 0.0 else np.full((128, 128), np.nan)
        fast = _gemm(gpu, ta, tb, alpha, A, B, beta, Cin, 128, 128, 32, 0)
        guarded = _gemm(gpu, ta, tb, alpha, A, B, beta, Cin, 128, 128, 32, 1)
        assert np.all(np.isfinite(fast)) and _same_bits(fast, guarded)
        assert _same_bits(fast, _gemm(gpu, ta, tb, alpha, A, B, beta, Cin, 128, 128, 32, 2))


# ===================================================================================== factor inverse
TRTRI_ORDERS = [1, 63, 64, 65, 128, 129, 192, 193, 257, 320, 513]


def _inverse_longdouble(L):
    """inv(L) by forward substitution in np.longdouble, row by row: X[i, :] = (e_i - L[i, :i] X[:i, :]) / L[i, i]"""
    n = L.shape[0]
    Lq = np.tril(L).astype(LD)
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        row = -(Lq[i, :i] @ X[:i, :i + 1]) if i else np.zeros(1, dtype=LD)
        row[i] += LD(1)
        X[i, :i + 1] = row / Lq[i, i]
    return X


@functools.lru_cache(maxsize=None)
def _factor_case(n):
    """(L with garbage above the diagonal, longdouble inverse, LAPACK dtrtri's error against it)"""
    rng = np.random.default_rng(n)
    G = rng.standard_normal((n + 20, n)) / np.sqrt(n + 20)  # as in test_trsv_pair: cond(G'G + I) < 10
    L = sla.cholesky(G.T @ G + np.eye(n), lower=True)
    ref = _inverse_longdouble(L)
    Xl, info = sla.lapack.dtrtri(np.asfortranarray(L), lower=1)
    assert info == 0
    scale = np.max(np.abs(ref))
    lapack_err = float(np.max(np.abs(np.tril(Xl).astype(LD) - ref)) / scale)
    Lg = np.asfortranarray(L + np.triu(rng.standard_normal((n, n)), 1))
    return Lg, ref, lapack_err


@functools.lru_cache(maxsize=None)
def _trtri_allowance():
    """8 x the largest error LAPACK's dtrtri makes on these matrices: recursive doubling stacks up to log2(n / 64) GEMM
    levels on the 64 x 64 block inverses, on matrices of condition number < 10"""
    return 8.0 * max(_factor_case(n)[2] for n in TRTRI_ORDERS)


def _trtri(gpu, L, n, ldL, ldX):
    Lb = _store(L, ldL, 123.0)
    Xb = np.full((ldX, n), SENTINEL, order="F")
    gpu._lib.check(gpu._lib.load().admm_op_trtri(_dp(gpu, Lb), n, ldL, _dp(gpu, Xb), ldX))
    # the launcher clears the whole ldX x n buffer (padded storage wants zero padding) and nothing may store there
    # afterwards: the sentinel is gone and the padding rows hold +0.0, bit for bit (a store past c_rows by a ragged
    # pair of the batched GEMMs would show here, -0.0 included)
    assert not np.any(_bits(Xb[n:])), "rows n .. ldX-1 of X are not +0.0: a kernel stored past the inverse's rows"
    return Xb[:n].copy()


@pytest.mark.parametrize("pad", [0, 5], ids=["ld=n", "ld=n+5"])
@pytest.mark.parametrize("n", TRTRI_ORDERS)
def test_trtri(gpu, n, pad):
    """inv(L) by recursive doubling: ragged last pairs (65, 129, 193, 257, 513), an unpaired last block (192, 320), odd
    leading dimensions (n + 5 for even n: the guarded loader inside the batched GEMMs).  The whole ldX x n buffer comes
    back: the padding rows must be +0.0 bits (cleared by the launcher, never stored to by a ragged pair).  The strict
    upper triangle is exactly zero and nothing is NaN: removing the zero_scratch_kernel launch leaves T' = X11' L21' above the diagonal
    (seen at every n > 64) and feeds it to the next level as part of X11 (the accuracy check, n > 128)."""
    L, ref, lapack_err = _factor_case(n)
    X = _trtri(gpu, L, n, n + pad, n + pad)
    assert not np.any(np.isnan(X))
    assert np.all(X[np.triu_indices(n, 1)] == 0.0)
    err = float(np.max(np.abs(X.astype(LD) - ref)) / np.max(np.abs(ref)))
    print(f"trtri n={n} ld=n+{pad}: kernel {err:.3e}  LAPACK {lapack_err:.3e}  allowance {_trtri_allowance():.3e}")
    assert err <= _trtri_allowance()


@pytest.mark.parametrize("n", [1, 64, 65, 129, 257])
def test_trtri_of_a_diagonal_is_exact(gpu, n):
    d = 2.0 ** ((np.arange(n) % 9) - 4)
    X = _trtri(gpu, np.asfortranarray(np.diag(d)), n, n, n)
    np.testing.assert_array_equal(X, np.diag(1.0 / d))


# ===================================================================================== y = L (L' x)
LLT_ORDERS = [1, 3, 63, 64, 65, 255, 256, 257, 600]


def _llt(gpu, L, n, x, ld):
    y = np.full(n, np.nan)
    gpu._lib.check(gpu._lib.load().admm_op_llt_apply(_dp(gpu, _lower_storage(L, ld)), n, ld, _dp(gpu, x), _dp(gpu, y)))
    return y


@pytest.mark.parametrize("n", LLT_ORDERS)
def test_llt_apply(gpu, n):
    """the probe's right-hand side y = L (L' x), NaN above the diagonal of L.  Exact: integers <= 2^10, so the two
    chained sums stay below n^2 2^30 < 2^53.  Bounded: t = L'x carries (n + 4) u |L'||x|, y = L t adds (n + 4) u |L||t|
    on top of |L| times the first error, and |t| <= |L'||x|:
        |y - ref| <= (2 g + g^2) |L| (|L'| |x|),   g = (n + 4) 2^-53."""
    rng = np.random.default_rng(n)
    Li = np.tril(rng.integers(-2 ** 10, 2 ** 10 + 1, (n, n)))
    xi = rng.integers(-2 ** 10, 2 ** 10 + 1, n)
    assert np.max(np.abs(Li) @ (np.abs(Li).T @ np.abs(xi))) < 2 ** 53
    ref = (Li @ (Li.T @ xi)).astype(np.float64)
    for ld in (n, n + 3):
        np.testing.assert_array_equal(_llt(gpu, Li.astype(np.float64), n, xi.astype(np.float64), ld), ref)
    L = np.tril(rng.standard_normal((n, n)))
    x = rng.standard_normal(n)
    Lq, xq = L.astype(LD), x.astype(LD)
    ref = Lq @ (Lq.T @ xq)
    g = (n + 4) * LD(U)
    bound = (2 * g + g * g) * (np.abs(Lq) @ (np.abs(Lq).T @ np.abs(xq)))
    assert _ratio(L @ (L.T @ x), ref, bound) <= 1.0  # NumPy's fp64 product obeys the bound
    worst = max(_ratio(_llt(gpu, L, n, x, ld), ref, bound) for ld in (n, n + 3))
    print(f"llt_apply n={n}: worst |err|/bound = {worst:.3f}")
    assert worst <= 1.0
