"""Host side of the operator tests of the spectral 2-D total-variation x-update (tests/test_gpu_tv2d_spectral.py):
the long-double references against a dense solve, the library's transform tables entry by entry, the row-stage
selection rule at its thresholds, and every bound the GPU tests assert, held against plain fp64 SciPy on the same
inputs -- a bound is then never tighter than fp64 allows.  No device."""
import numpy as np
import pytest
import scipy.fft
import scipy.linalg

import tv2d_spectral_restated as R

LD = R.LD


def _taps(ap, rho):
    t = ap._lib.load().admm_tv2d_rows_green_taps(float(rho))
    assert t > 0
    return t


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("H,W", [(8, 9), (9, 8)])
@pytest.mark.parametrize("rho", [1.0, 37.5])
def test_restatement_against_a_dense_solve(H, W, rho):
    """transform, row solve, inverse transform == inv(I + rho D'D) b with D from np.diff, in long double: pins the
    transform convention (no factor 2, see the module's docstring), the eigenvalues 4 sin^2(pi i/(2H)) and the Neumann
    ends of the row systems, independently of any kernel.  Both are long-double computations of ~100 operations per
    element on a system of condition <= 1 + 8 rho: 1e-16 relative is 2000 long-double roundings."""
    b = np.random.default_rng(H * W).standard_normal((H, W))
    x, _ = R.xsolve(b, rho)
    ref = R.dense_xsolve(b, rho)
    err = float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))
    print(f"restatement vs dense {H}x{W} rho={rho}: {err:.2e}")
    assert err <= 1e-16
    rt = R.idct2(R.dct2(b))
    assert float(np.max(np.abs(rt - b))) <= 1e-17
    fp = scipy.fft.dct(b, type=2, axis=0) / 2  # (SciPy carries a factor 2 the kernels do not)
    assert float(np.max(np.abs(fp - R.dct2(b)))) <= 1e-14


# ------------------------------------------------------------------------------------------------ tables
def _ulp_close(got, ref_ld):
    """|got - ref| <= 1 ulp of the reference rounded to double; at a zero of the closed form the long-double argument
    (pi rounded to 64 bits, times k/n) leaves a value below 2^-60 instead of 0: that much absolutely"""
    ref = np.asarray(ref_ld, dtype=np.float64)
    tol = np.maximum(np.spacing(np.abs(ref)), 2.0 ** -60)
    bad = np.abs(np.asarray(got, dtype=LD) - ref_ld) > tol
    return not bad.any(), int(np.argmax(bad))


@pytest.mark.parametrize("n", [8, 16, 4096, 8192, 9, 12, 1000, 2049, 4095])
def test_tables(ap, n):
    """Every entry of tw, c4, lam, chirp against the long-double closed form: these are long-double values rounded to
    double (1 ulp).  hbr is a radix-2 FFT of length M in long double (dct_fill_chirp_tables: cosl / sinl twiddles of a
    rounded angle, |dw| <= 14 E, E = 2^-64; eta <= 20 E; Higham Thm 24.2: ||dH||_2 <= log2(M) eta ||H||_2 <= 260 E
    sqrt(M (2n-1))), divided by M and rounded to double: |d hbr_p| <= sqrt2 u |hbr_p| + 300 E sqrt((2n-1)/M), the 300
    including 40 E for this reference's own pairwise sums."""
    t = R.library_tables(ap, n)
    chirp = not R.is_pow2(n)
    M = R.chirp_fft_length(n) if chirp else n
    assert len(t["tw"]) == M // 2 and len(t["lam"]) == n and len(t["c4"]) == (n if chirp else n // 2 + 1)
    k = np.arange(M // 2, dtype=np.int64)
    cm = R.cos_table(M)
    for name, got, ref in (("tw.re", t["tw"].real, cm[(4 * k) % (4 * M)]), ("tw.im", t["tw"].imag, -cm[(M - 4 * k) % (4 * M)])):
        ok, at = _ulp_close(got, ref)
        assert ok, (name, at, got[at], ref[at])
    cn = R.cos_table(n)
    k = np.arange(len(t["c4"]), dtype=np.int64)
    for name, got, ref in (("c4.re", t["c4"].real, cn[k]), ("c4.im", t["c4"].imag, -cn[(n - k) % (4 * n)])):
        ok, at = _ulp_close(got, ref)
        assert ok, (name, at, got[at], ref[at])
    k = np.arange(n, dtype=np.int64)
    ok, at = _ulp_close(t["lam"], LD(4) * cn[n - k] ** 2)
    assert ok and t["lam"][0] == 0.0, ("lam", at)
    if not chirp:
        assert len(t["chirp"]) == 0 and len(t["hbr"]) == 0
        return
    q = (k * k) % (2 * n)
    cr, ci = cn[(2 * q) % (4 * n)], -cn[(n - 2 * q) % (4 * n)]
    for name, got, ref in (("chirp.re", t["chirp"].real, cr), ("chirp.im", t["chirp"].imag, ci)):
        ok, at = _ulp_close(got, ref)
        assert ok, (name, at, got[at], ref[at])
    # h is even (h_m = h_(M-m) = conj(c_m), m < n): H_k = h_0 + 2 sum_{m=1}^{n-1} h_m cos(2 pi k m / M)
    hr, hi = cr.copy(), -ci
    hr[1:] *= 2
    hi = hi.copy()
    hi[1:] *= 2
    Hr, Hi = np.empty(M, dtype=LD), np.empty(M, dtype=LD)
    step = max(1, (1 << 21) // n)
    for k0 in range(0, M, step):
        kk = np.arange(k0, min(M, k0 + step), dtype=np.int64)
        c = cm[(4 * np.outer(kk, k)) % (4 * M)]
        Hr[kk], Hi[kk] = (c * hr).sum(axis=1), (c * hi).sum(axis=1)
    L = R.log2i(M)
    brev = np.array([int(format(p, f"0{L}b")[::-1], 2) for p in range(M)])
    ref_r, ref_i = Hr[brev] / M, Hi[brev] / M
    mag = np.sqrt(ref_r ** 2 + ref_i ** 2)
    tol = np.sqrt(LD(2)) * R.U * mag + R.HBR_LD_TERM * np.sqrt(LD(2 * n - 1) / M)
    err = np.sqrt((t["hbr"].real - ref_r) ** 2 + (t["hbr"].imag - ref_i) ** 2)
    print(f"hbr n={n}: worst error/bound {float(np.max(err / tol)):.3f}")
    assert np.all(err <= tol)


# ------------------------------------------------------------------------------------------------ the selection rule
def _rho_with_taps(ap, want):
    """the largest rho on a fine grid whose truncation is `want` terms (the count grows with rho)"""
    lo, hi = 1e-3, 50.0
    assert _taps(ap, lo) < want < _taps(ap, hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if _taps(ap, mid) <= want:
            lo = mid
        else:
            hi = mid
    assert _taps(ap, lo) == want and _taps(ap, hi) == want + 1
    return lo, hi


def test_selection_rule_at_its_thresholds(ap):
    """Expected forms written down from the comments of dct.hip: the Toeplitz stage while its truncation t is at most 96
    terms and 4 t <= W; of its two kernels the cooperative one when t <= 64 (its two 32-column halo runs) and W >= 384
    (its 12 output runs); else the row transform where W is a power of two and H is even (row PAIRS); else Thomas."""
    L = ap._lib
    stage = lambda H, W, rho: L.load().admm_tv2d_row_stage(H, W, float(rho))
    G, C, D, T = L.TV2D_ROWS_GREEN, L.TV2D_ROWS_COOP, L.TV2D_ROWS_DCT, L.TV2D_ROWS_THOMAS
    t = _taps(ap, 1.0)
    assert t <= 64 and 4 * t < 383
    assert stage(64, 4 * t - 1, 1.0) == T and stage(64, 4 * t, 1.0) == G
    r96, r97 = _rho_with_taps(ap, 96)
    assert stage(64, 4 * 96, r96) == G          # (t = 96 > 64: never cooperative)
    assert stage(64, 4 * 97, r97) == T          # t = 97: no Toeplitz stage at any width ...
    assert stage(64, 1024, r97) == D and stage(64, 1024, r96) == G and stage(64, 100000, r97) == T
    r64, r65 = _rho_with_taps(ap, 64)
    assert stage(64, 384, r64) == C and stage(64, 384, r65) == G
    assert stage(64, 383, 1.0) == G and stage(64, 384, 1.0) == C
    assert stage(63, 383, 1.0) == G and stage(65, 384, 1.0) == C  # (the Toeplitz kernels take any height)
    assert stage(64, 64, 1.0) == D and stage(63, 64, 1.0) == T and stage(65, 64, 1.0) == T
    assert stage(64, 1, 1.0) == T and stage(9, 1, 1.0) == T and stage(64, 1, 1e-3) == T
    assert stage(7, 64, 1.0) == L.TV2D_ROWS_AUTO and stage(8193, 64, 1.0) == L.TV2D_ROWS_AUTO  # CG: no row stage
    for bad in ((0, 8, 1.0), (8, 0, 1.0), (8, 8, 0.0), (8, 8, -1.0), (8, 8, float("nan")), (8, 8, float("inf"))):
        assert stage(*bad) == L.E_INVALID, bad


def test_spectral_ops_reject_bad_arguments_before_touching_the_device(ap):
    """E_INVALID decided on the host -- the same answer with and without a device -- and the output stays untouched"""
    ops, (a, o) = R.spectral_op_calls(ap)
    for name, kw in R.spectral_bad_calls():
        assert ops[name](**kw) == ap._lib.E_INVALID, (name, kw)
    assert np.all(np.isnan(o))
    for name in ops:
        assert f"admm_op_{name}" in ap._lib.EXPORTED_SYMBOLS
    expected = ap._lib.OK if ap._lib.device_count() > 0 else ap._lib.E_DEVICE  # valid arguments: a device, or E_DEVICE
    for name, call in ops.items():
        assert call() == expected, name


# ------------------------------------------------------------------------------------------------ fp64 inside the bounds
@pytest.mark.parametrize("H", R.NET_HEIGHTS + R.CHIRP_HEIGHTS)
def test_column_bounds_hold_for_fp64_scipy(ap, H):
    """scipy.fft.dct / idct (type 2, norm=None, pocketfft in fp64) on the inputs of the GPU test, inside the bounds the
    GPU test asserts of the kernels, at every width"""
    hmax = R.hbr_max(ap, H)
    worst = 0.0
    for inverse in (False, True):
        for name, (x, ref) in R.col_reference(H, inverse).items():
            got = scipy.fft.idct(2 * x, type=2, axis=0) if inverse else scipy.fft.dct(x, type=2, axis=0) / 2
            err = np.sqrt(np.sum((got - ref) ** 2, axis=0))
            for W in R.COL_WIDTHS:
                if W > x.shape[1]:
                    continue
                bound = R.col_bound(H, inverse, x[:, :W], ref[:, :W], hmax)
                worst = max(worst, float(np.max(err[:W] / bound)))
    print(f"fp64 columns H={H}: worst error/bound {worst:.4f}")
    assert worst <= 1.0


def _fp64_rows(b, rho, lam):
    H, W = b.shape
    out = np.empty((H, W))
    for i in range(H):
        d = 1.0 + rho * (lam[i] + 2.0)
        ab = np.zeros((3, W))
        ab[0, 1:] = -rho
        ab[2, :-1] = -rho
        ab[1] = d
        ab[1, 0] -= rho
        ab[1, -1] -= rho
        out[i] = scipy.linalg.solve_banded((1, 1), ab, b[i])
    return out


def _fp64_rows_by_transform(b, rho, lam, lam_w):
    X = scipy.fft.dct(b, type=2, axis=1) / 2
    X /= 1.0 + rho * (lam[:b.shape[0], None] + lam_w[None, :])
    return scipy.fft.idct(2 * X, type=2, axis=1)


def test_row_bounds_hold_for_fp64_solve_banded(ap):
    """scipy.linalg.solve_banded (LAPACK dgtsv, fp64) on every input of the forced row-stage tests, inside the bound
    of the form the GPU test forces there.  The bound of the DCT form is that of a spectral division, which does not
    grow with the condition 1 + 4 rho of a row system; an elimination's error does (solve_banded is 1.14 x that bound
    at 8 x 8192, rho = 1e4, and far more at 1e6).  For that form the fp64 counterpart is therefore the same algorithm
    in fp64 SciPy -- dct along the row, division, idct -- and solve_banded is held to it where rho <= 5."""
    worst = {}
    for form, H, W, rho in R.row_cases(lambda rho: _taps(ap, rho)):
        lam = R.library_tables(ap, H)["lam"]
        b = R.row_input(H, W)
        ref = R.row_solve(b, rho, lam)
        if form == R.ROWS_DCT:
            got = _fp64_rows(b, rho, lam) if rho <= 5 else _fp64_rows_by_transform(b, rho, lam, R.library_tables(ap, W)["lam"])
            err = R.pair_error(got - ref)
        else:
            err = np.abs(_fp64_rows(b, rho, lam) - ref)
        ratio = float(np.max(err / R.row_bound(form, b, ref, rho, lam, _taps(ap, rho))))
        worst[form] = max(worst.get(form, 0.0), ratio)
        assert ratio <= 1.0, (form, H, W, rho, ratio)
    print("fp64 rows, worst error/bound per form (1 green, 2 coop, 3 dct, 4 thomas):", worst)


@pytest.mark.parametrize("H,W", R.XSOLVE_SHAPES)
def test_xsolve_bound_holds_for_fp64(ap, H, W):
    """the composition in fp64 SciPy inside the composed bound, with the row stage the rule names at each rho"""
    lam = R.library_tables(ap, H)["lam"]
    b = R.xsolve_input(H, W)
    for rho in R.XSOLVE_RHOS:
        form = ap._lib.load().admm_tv2d_row_stage(H, W, rho)
        ref, bh = R.xsolve(b, rho, lam)
        got = scipy.fft.idct(2 * _fp64_rows(scipy.fft.dct(b, type=2, axis=0) / 2, rho, lam), type=2, axis=0)
        bound = R.xsolve_bound(H, W, form, b, bh, ref, rho, lam, _taps(ap, rho), R.hbr_max(ap, H))
        ratio = float(np.sqrt(np.sum((got - ref) ** 2)) / bound)
        print(f"fp64 xsolve {H}x{W} rho={rho} form={form}: error/bound {ratio:.4f}")
        assert ratio <= 1.0
