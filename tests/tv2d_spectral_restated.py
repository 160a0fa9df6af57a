"""Long-double restatement of the spectral x-update of 2-D total variation (csrc/dct.hip), the error bounds its
operator tests assert, and the inputs those tests use.  Pure NumPy; the library is called by library_tables alone,
which hands back its host tables.

Conventions (found in the code, which is the contract): the forward column transform is the DCT-II WITHOUT the factor 2
of scipy.fft.dct(type=2, norm=None):  X_k = sum_j x_j cos(pi k (2j+1) / (2n));  the inverse is its exact inverse
x_j = (X_0 + 2 sum_{k>=1} X_k cos(pi k (2j+1)/(2n))) / n.  dct.h says "unnormalised" for the first and "DCT-III with the
1/H factor" for the second; both are these.

Error model (u = 2^-53).  Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 24.2: a radix-2 FFT of
length N = 2^L with twiddles accurate to mu has  ||dy||_2 <= L eta ||y||_2 / (1 - L eta),  eta = mu + gamma_4 (sqrt2 + mu).
The table test proves every twiddle component within 1 ulp, so |dw| <= sqrt2 u; a fused pass forms some twiddles as the
product of a table entry and a 16th root of unity given to 20 digits (sqrt2 u each, plus 2 sqrt2 u for the complex
product): mu = 4 sqrt2 u, eta <= 12 u.  Second-order terms are below 1e-12 of every bound and are covered by rounding the
constants up.
  Network, forward: the two columns of a pair are one complex sequence z, ||Z||_2 = sqrt(n) ||z||_2 =: S.  The even/odd
  split is one addition and an exact halving per component (u), the c4 rotation a complex product with a 1-ulp entry
  (sqrt2 u + 2 sqrt2 u), the scale at k = n/2 one product: jointly over the pair
  ||dX||_2 <= (12 L + 5.25) u S.  Inverse: rotation, one addition (7.01 u ||Z||), the network, an exact 1/n:
  ||dx||_2 <= (12 L + 7.01) u ||x_pair||_2.  One constant for both:  C_NET(n) = 12 log2(n) + 8.
  Chirp form, bm = 2^Lb: chirp product (4.25 u), FFT (12 Lb u), pointwise product with hbr (2 sqrt2 u and the table's
  own error, test_tables: c_h), inverse FFT (12 Lb u), chirp product (4.25 u), then the split and rotation (5.25 u), or
  in the inverse direction rotation, addition, chirp in front (9.5 u) and the 1/n scale behind (u): all relative to the
  norm of the convolution's intermediates, at most bm max|hbr| ||z||_2:
  C_CHIRP = 24 Lb + 24 + c_h  against the scale  max(bm max|hbr|, sqrt n) ||z||_2  (inverse: divided by sqrt n).
Row stages: the bound is element-wise,  |err| <= c u inv(A) (|A||x| + |b|)  with A = tridiag(-rho, d_i, -rho), end entries
d_i - rho: A is an M-matrix, inv(A) >= 0, and the right-hand side is one more long-double solve.
  THOMAS: Higham Thm 9.14 with Thm 9.12 for a diagonally dominant tridiagonal matrix: (A + dA) xhat = b with
  |dA| <= 3 f(u) |A|, f(u) = 4u + O(u^2) for a division per row.  The kernel multiplies by a stored reciprocal and stores
  the rounded c' = -rho r (one more rounding in each of the two: f -> 6u):  C_THOMAS = 18.  It also forms
  d_i = 1 + rho (lam_i + 2) and the end entries d_i - rho (W = 1: d_i - 2 rho = 1 + rho lam_i, a cancellation) in fp64:
  four roundings of size u d_i in a diagonal entry that can be as small as 1, i.e. |dA_jj| <= 4 u d_i and not 4 u |A_jj|
  (the first version of this bound said the latter, and fp64 solve_banded broke it 2.9-fold at W = 1, rho = 300):
  + 4 u inv(A) (d_i |x|), one more solve.
  GREEN: x_j = A_i sum_m r^|m| b_mirror(j+m).  r = 2 rho / (d + sqrt(d^2 - 4 rho^2)): for rho <= 5 (the forced rhos)
  d^2 / (d^2 - 4 rho^2) <= 121/21, so the discriminant has relative error <= 3 * 5.8 u, its root 10 u, A = 1/root 11 u,
  and r <= 6 u =: d_r.  A term at distance m carries r^m (m d_r) and passes m + 1 fused multiply-adds (one rounding
  each), and the recurrences reach back over the truncation K plus the 128 columns of a wave's four runs:
  C_GREEN(K) = 7 (K + 128) + 16.  What the truncation and the single reflection leave out is below
  4e-18 A_i max_j|b_ij| / (1 - r_i), added as an absolute term.
  COOP: carries cross two 32-column runs through r^32 (five squarings), chains of at most 96 + 8 terms:
  C_COOP = 7 * 104 + 16 = 744; and the anticausal pass rebuilds b_(t+1) = c_(t+1) - r c_t, one rounding of size u |c| per
  column, |c| <= inv(A)|b| / A_i, which the recurrence sums once more:  + 2 u sqrt(d^2 - 4 rho^2) inv(A) inv(A) |b|.
  DCT: a transform solve has no element-wise bound; norm-wise per row pair, the transform bound twice plus the division
  (denominator: four roundings, quotient: one; every denominator >= 1, ||inverse transform|| = sqrt(2/W)):
  ||err_pair||_2 <= u (2 (C_NET(W) + 5) ||b_pair||_2 + C_NET(W) ||x_pair||_2).
"""
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
PI = LD(4) * np.arctan(LD(1))
NAN_FILL = np.float64(np.nan)

ROWS_AUTO, ROWS_GREEN, ROWS_COOP, ROWS_DCT, ROWS_THOMAS = range(5)


# ------------------------------------------------------------------------------------------------ transforms
@functools.lru_cache(maxsize=None)
def cos_table(n):
    """cos(pi m / (2n)), m < 4n, long double; first quadrant evaluated, the rest by symmetry (exact zeros and ones)"""
    m = np.arange(n + 1, dtype=LD)
    q = np.cos(PI * m / LD(2 * n))
    q[n] = LD(0)
    t = np.empty(4 * n, dtype=LD)
    t[:n + 1] = q
    t[n + 1:2 * n + 1] = -q[n - 1::-1]   # cos(pi - a) = -cos a
    t[2 * n + 1:] = t[2 * n - 1:0:-1]    # cos(2 pi - a) = cos a
    return t


def _product(n, x, transpose):
    """sum over the second (transpose: first) index of cos(pi k (2j+1)/(2n)) x, in row chunks"""
    x = np.asarray(x, dtype=LD).reshape(n, -1)
    t = cos_table(n)
    odd = 2 * np.arange(n, dtype=np.int64) + 1
    out = np.empty_like(x)
    step = max(1, (1 << 21) // n)
    for r0 in range(0, n, step):
        r = np.arange(r0, min(n, r0 + step), dtype=np.int64)
        idx = (np.outer(odd[r], np.arange(n, dtype=np.int64)) if transpose else np.outer(r, odd)) % (4 * n)
        out[r] = t[idx] @ x
    return out


def dct2(x):
    """X_k = sum_j x_j cos(pi k (2j+1)/(2n)) along axis 0, long double"""
    x = np.asarray(x, dtype=LD)
    return _product(x.shape[0], x, False).reshape(x.shape)


def idct2(X):
    """the inverse of dct2 along axis 0"""
    X = np.asarray(X, dtype=LD)
    n = X.shape[0]
    w = np.full(n, LD(2))
    w[0] = LD(1)
    Xw = X * w.reshape((n,) + (1,) * (X.ndim - 1))
    return (_product(n, Xw, True) / LD(n)).reshape(X.shape)


def dct2_of_unit(n, j):
    return cos_table(n)[(np.arange(n, dtype=np.int64) * (2 * j + 1)) % (4 * n)].copy()


def lam_exact(n):
    s = np.sin(PI * np.arange(n, dtype=LD) / LD(2 * n))
    return LD(4) * s * s


# ------------------------------------------------------------------------------------------------ row systems
def _diag(H, W, rho, lam):
    rho = LD(rho)
    d = LD(1) + rho * (np.asarray(lam, dtype=LD)[:H] + LD(2))
    D = np.repeat(d[:, None], W, axis=1)
    D[:, 0] -= rho
    D[:, W - 1] -= rho
    return D


def row_solve(b, rho, lam):
    """every row i of b (H x W) through inv(tridiag(-rho, d_i, -rho)), ends d_i - rho: long-double Thomas"""
    b = np.asarray(b, dtype=LD)
    H, W = b.shape
    D, rho = _diag(H, W, rho, lam), LD(rho)
    cp = np.zeros((H, W), dtype=LD)
    dp = np.zeros((H, W), dtype=LD)
    c_prev, d_prev = np.zeros(H, dtype=LD), np.zeros(H, dtype=LD)
    for j in range(W):
        den = D[:, j] + rho * c_prev
        c_prev = -rho / den
        d_prev = (b[:, j] + rho * d_prev) / den
        cp[:, j], dp[:, j] = c_prev, d_prev
    x = np.empty((H, W), dtype=LD)
    x[:, W - 1] = dp[:, W - 1]
    for j in range(W - 2, -1, -1):
        x[:, j] = dp[:, j] - cp[:, j] * x[:, j + 1]
    return x


def row_apply_abs(x, rho, lam):
    """|A| |x| row by row"""
    x = np.abs(np.asarray(x, dtype=LD))
    H, W = x.shape
    y = _diag(H, W, rho, lam) * x
    y[:, 1:] += LD(rho) * x[:, :-1]
    y[:, :-1] += LD(rho) * x[:, 1:]
    return y


def dense_solve(A, b):
    """long-double Gaussian elimination without pivoting (A symmetric positive definite)"""
    A = np.array(A, dtype=LD)
    b = np.array(b, dtype=LD)
    n = A.shape[0]
    for k in range(n - 1):
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= np.outer(f, A[k, k:])
        b[k + 1:] -= f * b[k]
    x = np.empty(n, dtype=LD)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def dense_xsolve(b, rho):
    """inv(I + rho D'D) b for the image b, D the stacked vertical and horizontal differences (np.diff)"""
    H, W = b.shape
    N = H * W
    I = np.eye(N).reshape(N, H, W)
    Dv = np.diff(I, axis=1).reshape(N, -1).T
    Dh = np.diff(I, axis=2).reshape(N, -1).T
    A = np.eye(N, dtype=LD) + LD(rho) * (Dv.T @ Dv + Dh.T @ Dh).astype(LD)
    return dense_solve(A, np.asarray(b, dtype=LD).reshape(-1)).reshape(H, W)


def xsolve(b, rho, lam=None):
    """transform, row solve, inverse transform in long double (lam: the library's table, or the exact eigenvalues)"""
    H = b.shape[0]
    bh = dct2(b)
    return idct2(row_solve(bh, rho, lam_exact(H) if lam is None else lam)), bh


# ------------------------------------------------------------------------------------------------ bounds
def log2i(n):
    return int(n).bit_length() - 1


def is_pow2(n):
    return n & (n - 1) == 0


def chirp_fft_length(n):
    m = 16
    while m < 2 * n - 1:
        m <<= 1
    return m


HBR_LD_TERM = 300.0 * 2.0 ** -64  # test_tables: the long-double FFT behind hbr, absolute, times sqrt((2n-1)/bm)


def c_net(n):
    return 12.0 * log2i(n) + 8.0


def col_constants(H, hbr_max=None):
    """(c, forward scale per unit ||z||_2, inverse scale per unit ||x_pair||_2) of the column transform of length H;
    hbr_max = max |hbr| of the library's table (chirp lengths)"""
    if is_pow2(H):
        return c_net(H), float(np.sqrt(H)), 1.0
    M = chirp_fft_length(H)
    c_h = np.sqrt(2.0) + HBR_LD_TERM * np.sqrt((2 * H - 1) / M) / (U * hbr_max)
    conv = max(M * hbr_max, np.sqrt(H))
    return 24.0 * log2i(M) + 24.0 + c_h, float(conv), float(conv / np.sqrt(H))


def pair_norms(x):
    """per column: the 2-norm of the column pair it is transformed with (an odd width's last column: itself twice)"""
    x = np.asarray(x, dtype=LD)
    W = x.shape[1]
    sq = np.sum(x * x, axis=0)
    out = np.empty(W, dtype=LD)
    for j in range(0, W, 2):
        out[j:j + 2] = np.sqrt(sq[j] + sq[j + 1]) if j + 1 < W else np.sqrt(2 * sq[j])
    return out


def col_bound(H, inverse, inp, ref, hbr_max=None):
    """per column: the bound on ||got - ref||_2"""
    c, sf, si = col_constants(H, hbr_max)
    return c * U * (si * pair_norms(ref) if inverse else sf * pair_norms(inp))


C_THOMAS = 18.0


def c_green(taps):
    return 7.0 * (taps + 128) + 16.0


C_COOP = 7.0 * 104 + 16.0


def row_bound(form, b, x, rho, lam, taps):
    """element-wise (DCT: per row pair, every element of the pair carrying the pair's norm-wise bound) bound on
    |got - x| for the row stage `form`; b, x long double, x = row_solve(b)"""
    b, x = np.asarray(b, dtype=LD), np.asarray(x, dtype=LD)
    H, W = b.shape
    if form == ROWS_DCT:
        c = c_net(W)
        out = np.empty((H, W), dtype=LD)
        for i in range(0, H, 2):
            nb = np.sqrt(np.sum(b[i:i + 2] ** 2))
            nx = np.sqrt(np.sum(x[i:i + 2] ** 2))
            out[i:i + 2] = U * (2 * (c + 5) * nb + c * nx)
        return out  # compare with the pair's 2-norm of the error, not element-wise
    base = row_solve(row_apply_abs(x, rho, lam) + np.abs(b), rho, lam)
    d = LD(1) + LD(rho) * (np.asarray(lam, dtype=LD)[:H] + LD(2))
    if form == ROWS_THOMAS:
        return C_THOMAS * U * base + 4 * U * row_solve(d[:, None] * np.abs(x), rho, lam)
    disc = np.sqrt(d * d - LD(4) * LD(rho) * LD(rho))
    r = LD(2) * LD(rho) / (d + disc)
    trunc = (LD(4e-18) / ((LD(1) - r) * disc) * np.max(np.abs(b), axis=1))[:, None]
    if form == ROWS_GREEN:
        return c_green(taps) * U * base + trunc
    twice = row_solve(row_solve(np.abs(b), rho, lam), rho, lam)
    return C_COOP * U * base + 2 * U * disc[:, None] * twice + trunc


def xsolve_bound(H, W, form, b, bh, x, rho, lam, taps, hbr_max=None):
    """Frobenius-norm bound of the composed x-solve: the forward error through the row operator (norm <= 1) and the
    inverse transform (norm sqrt(2/H)), the row stage's own bound the same way, the inverse transform's error"""
    c, sf, si = col_constants(H, hbr_max)
    fro = lambda a: np.sqrt(np.sum(np.asarray(a, dtype=LD) ** 2))
    fwd = c * U * sf * np.sqrt(LD(2)) * fro(b)
    rows = row_bound(form, bh, row_solve(bh, rho, lam), rho, lam, taps)
    rows = fro(rows[::2, 0]) if form == ROWS_DCT else fro(rows)  # (DCT: one norm-wise figure per row pair)
    return np.sqrt(LD(2) / H) * (fwd + rows) + c * U * si * np.sqrt(LD(2)) * fro(x)


def pair_error(err):
    """the 2-norm of the error over every row pair, shaped like row_bound's DCT result"""
    err = np.asarray(err, dtype=LD)
    out = np.empty_like(err)
    for i in range(0, err.shape[0], 2):
        out[i:i + 2] = np.sqrt(np.sum(err[i:i + 2] ** 2))
    return out


@functools.lru_cache(maxsize=None)
def _tables_cached(lib_mod, n):
    import ctypes as C
    lib = lib_mod.load()
    counts = (C.c_int64 * 5)()
    lib_mod.check(lib.admm_dct_tables(n, None, None, None, None, None, counts))
    width = (2, 2, 1, 2, 2)
    bufs = [np.full(max(1, int(c)) * w, np.nan) for c, w in zip(counts, width)]
    lib_mod.check(lib.admm_dct_tables(n, *[lib_mod.as_dp(b) for b in bufs], counts))
    out = {}
    for name, c, w, b in zip(("tw", "c4", "lam", "chirp", "hbr"), counts, width, bufs):
        b = b[:int(c) * w]
        out[name] = b if w == 1 else b[0::2] + 1j * b[1::2]
    return out


def library_tables(ap, n):
    """the host tables of length n as admm_dct_tables returns them: complex tw, c4, chirp, hbr and real lam"""
    return _tables_cached(ap._lib, int(n))


def hbr_max(ap, n):
    return None if is_pow2(n) else float(np.max(np.abs(library_tables(ap, n)["hbr"])))


# ------------------------------------------------------------------------------------------------ cases
NET_HEIGHTS = (8, 16, 32, 64, 128, 256, 4096, 8192)
CHIRP_HEIGHTS = (9, 12, 17, 100, 1000, 2049, 4095)
COL_WIDTHS = (1, 2, 3, 5)


def col_inputs(H):
    """{name: H x k image}: standard normal (5 columns: every width takes the first W), the unit vectors e_j at
    j = 0, 1, H/2, H-1, one cosine mode"""
    rng = np.random.default_rng(1000 + H)
    units = np.zeros((H, 4))
    for c, j in enumerate(unit_indices(H)):
        units[j, c] = 1.0
    k = max(1, H // 3)
    mode = np.cos(np.pi * k * (2 * np.arange(H) + 1) / (2 * H)).reshape(H, 1)
    return dict(normal=rng.standard_normal((H, 5)), unit=units, mode=mode)


def unit_indices(H):
    return (0, 1, H // 2, H - 1)


@functools.lru_cache(maxsize=None)
def col_reference(H, inverse):
    """{name: (input, long-double result)} of col_inputs(H), computed once"""
    out = {}
    for name, x in col_inputs(H).items():
        if name == "unit" and not inverse:
            ref = np.stack([dct2_of_unit(H, j) for j in unit_indices(H)], axis=1)
        elif name == "unit":
            odd = 2 * np.arange(H, dtype=np.int64) + 1  # x_j = w_k cos(pi k (2j+1)/(2H)) / H, w_0 = 1, else 2
            ref = np.stack([LD(1 if k == 0 else 2) * cos_table(H)[(k * odd) % (4 * H)] / LD(H)
                            for k in unit_indices(H)], axis=1)
        else:
            ref = idct2(x) if inverse else dct2(x)
        out[name] = (x, ref)
    return out


ROW_HEIGHTS = (8, 64, 63, 65)
RHOS = (1e-3, 0.3, 1.0, 2.0, 5.0)
RHOS_LARGE = (300.0, 1e4, 1e6)


def row_cases(taps_of):
    """[(form, H, W, rho)] of the forced row-stage tests; taps_of(rho) = the library's truncation"""
    cases = []
    for rho in RHOS:
        t = taps_of(rho)
        green = {4 * t, 4 * t + 1} | {w for w in (127, 128, 129, 511, 512, 513) if w >= 4 * t}
        if 65 <= t <= 96:
            green |= {384, 513}
        coop = [w for w in (384, 385, 767, 768, 769) if t <= 64]
        for H in ROW_HEIGHTS:
            cases += [(ROWS_GREEN, H, w, rho) for w in sorted(green) if t < w]
            cases += [(ROWS_COOP, H, w, rho) for w in coop]
    for rho in RHOS + RHOS_LARGE:
        for H in ROW_HEIGHTS:
            cases += [(ROWS_THOMAS, H, w, rho) for w in (1, 2, 15, 16, 17, 33, 255)]
            if H % 2 == 0:
                cases += [(ROWS_DCT, H, w, rho) for w in (8, 16, 64, 1024, 8192)]
    return cases


def row_input(H, W):
    return np.random.default_rng(7 * H + W).standard_normal((H, W))


XSOLVE_SHAPES = ((8, 8), (64, 32), (9, 200), (100, 17), (64, 384), (2049, 8), (8192, 8), (8, 8192), (33, 1), (8, 1))
XSOLVE_RHOS = (1.0, 2381.0)
XSOLVE_DENSE = ((8, 8), (8, 1), (33, 1))


def xsolve_input(H, W):
    return np.random.default_rng(H + 31 * W).standard_normal((H, W))


# ------------------------------------------------------------------------------------------------ argument errors
def spectral_op_calls(ap):
    """(name -> call(**overrides) -> rc) of the three device operators with valid 8 x 8 arguments, and the arrays"""
    L, dp = ap._lib.load(), ap._lib.as_dp
    # 16 x 512 behind every pointer although the valid call is 8 x 8: should a library ever accept one of the calls of
    # spectral_bad_calls that only its rule refuses (H <= 9, W <= 384), it finds room and the test fails on the return
    # code, not on a heap it overran
    a, o = np.ones(16 * 512), np.full(16 * 512, np.nan)

    def dct_cols(img=dp(a), H=8, W=8, inverse=0, out=dp(o)):
        return L.admm_op_dct_cols(img, H, W, inverse, out)

    def tv2d_rows(src=dp(a), H=8, W=8, rho=1.0, form=0, out=dp(o)):
        return L.admm_op_tv2d_rows(src, H, W, rho, form, out)

    def tv2d_xsolve(b=dp(a), H=8, W=8, rho=1.0, form=0, x=dp(o)):
        return L.admm_op_tv2d_xsolve(b, H, W, rho, form, x)

    return dict(dct_cols=dct_cols, tv2d_rows=tv2d_rows, tv2d_xsolve=tv2d_xsolve), (a, o)


def spectral_bad_calls():
    bad = [(op, dict(H=h)) for op in ("dct_cols", "tv2d_rows", "tv2d_xsolve") for h in (7, 8193, 5000, 0)]
    bad += [(op, dict(W=0)) for op in ("dct_cols", "tv2d_rows", "tv2d_xsolve")]
    bad += [(op, dict(rho=r)) for op in ("tv2d_rows", "tv2d_xsolve") for r in (0.0, -1.0, float("nan"), float("inf"))]
    bad += [(op, dict(form=f)) for op in ("tv2d_rows", "tv2d_xsolve") for f in (-1, 5)]
    bad += [("dct_cols", dict(img=None)), ("dct_cols", dict(out=None)), ("dct_cols", dict(inverse=2)),
            ("tv2d_rows", dict(src=None)), ("tv2d_rows", dict(out=None)),
            ("tv2d_xsolve", dict(b=None)), ("tv2d_xsolve", dict(x=None))]
    # a forced form outside its own precondition: truncation (45 terms at rho = 1) >= W; below 384 columns; more than
    # 64 terms (rho = 5); a width without a row transform; an odd height
    bad += [(op, kw) for op in ("tv2d_rows", "tv2d_xsolve") for kw in (
        dict(form=1, W=8), dict(form=2, W=8), dict(form=2, W=383), dict(form=2, W=384, rho=5.0), dict(form=3, W=12),
        dict(form=3, H=9, W=8))]
    return bad
