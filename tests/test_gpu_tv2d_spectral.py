"""The kernels of the spectral 2-D total-variation x-update (csrc/dct.hip), each on its own through the operator
entry points admm_op_dct_cols, admm_op_tv2d_rows and admm_op_tv2d_xsolve, against the long-double restatement and
inside the a-priori bounds of tests/tv2d_spectral_restated.py (derived there; no constant is measured, and
tests/test_tv2d_spectral_host.py holds fp64 SciPy to the same bounds on the same inputs).  Outputs start as NaN, the
device images lie between guard columns the operators check (a write outside the image is E_NUMERIC), and every test
prints its worst error/bound ratio."""
import numpy as np
import pytest

import tv2d_spectral_restated as R

pytestmark = pytest.mark.gpu
LD = R.LD


def _f(a):
    return np.asfortranarray(a, dtype=np.float64)


def _cols(gpu, img, inverse):
    img = _f(img)
    H, W = img.shape
    out = np.full((H, W), np.nan, order="F")
    gpu._lib.check(gpu._lib.load().admm_op_dct_cols(gpu._lib.as_dp(img), H, W, int(inverse), gpu._lib.as_dp(out)))
    assert not np.isnan(out).any()
    return out


def _rows(gpu, src, rho, form, xsolve=False):
    src = _f(src)
    H, W = src.shape
    out = np.full((H, W), np.nan, order="F")
    fn = gpu._lib.load().admm_op_tv2d_xsolve if xsolve else gpu._lib.load().admm_op_tv2d_rows
    gpu._lib.check(fn(gpu._lib.as_dp(src), H, W, float(rho), int(form), gpu._lib.as_dp(out)))
    assert not np.isnan(out).any()
    return out


def _taps(gpu, rho):
    return gpu._lib.load().admm_tv2d_rows_green_taps(float(rho))


def _colnorm(a):
    return np.sqrt(np.sum(np.asarray(a, dtype=LD) ** 2, axis=0))


# ------------------------------------------------------------------------------------------------ column transform
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("H", R.NET_HEIGHTS + R.CHIRP_HEIGHTS)
def test_column_transform(gpu, H, inverse):
    """Every radix plan of the network (H = 8 .. 128: rem = 3, 0, 1, 2, 3; 256 and 4096: two and three radix-16 passes;
    8192: 128 KB of LDS) and the chirp form (9, 12, 17: smallest and odd; 2049: the 512-thread block; 4095), at widths
    1, 2, 3, 5, on standard-normal columns, the unit vectors e_0, e_1, e_(H/2), e_(H-1) (the answer is one cosine column:
    a misrouted Makhoul, bit-reverse or swizzle index shows) and one cosine mode (a spike and rounding).  Per column
    ||got - ref||_2 <= C u scale, C = 12 log2(H) + 8 (network) or 24 log2(bm) + 24 + c_h (chirp), derived in
    tv2d_spectral_restated.py from Higham Thm 24.2.  Also: a second call repeats the first bit for bit, an odd width's
    last column has the bits it gets in an even-width image that holds it twice, and forward then inverse returns the
    input within twice the bound (the issue's figure; the operator norms would allow 1 + sqrt2)."""
    hmax = R.hbr_max(gpu, H)
    refs = R.col_reference(H, inverse)
    worst = 0.0
    for name, (x, ref) in refs.items():
        widths = [w for w in R.COL_WIDTHS if w <= x.shape[1]] + ([4] if name == "unit" else [])
        for W in widths:
            got = _cols(gpu, x[:, :W], inverse)
            bound = R.col_bound(H, inverse, x[:, :W], ref[:, :W], hmax)
            ratio = float(np.max(_colnorm(got - ref[:, :W]) / bound))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, W, ratio)
    x = refs["normal"][0]
    a = _cols(gpu, x, inverse)
    assert np.array_equal(a, _cols(gpu, x, inverse))
    odd, even = _cols(gpu, x[:, :3], inverse), _cols(gpu, x[:, [0, 1, 2, 2]], inverse)
    assert np.array_equal(odd, even[:, :3])  # (the second half, even[:, 3], agrees with it to rounding only)
    one = _cols(gpu, x[:, :1], inverse)
    assert np.array_equal(one[:, 0], _cols(gpu, x[:, [0, 0]], inverse)[:, 0])
    if not inverse:
        back = _cols(gpu, a, True)
        c, _, si = R.col_constants(H, hmax)
        rt = float(np.max(_colnorm(back - x) / (2 * c * R.U * si * R.pair_norms(x))))
        print(f"columns H={H}: round trip error / (2 x bound) {rt:.4f}")
        assert rt <= 1.0
    print(f"columns H={H} {'inverse' if inverse else 'forward'}: worst error/bound {worst:.4f}")


# ------------------------------------------------------------------------------------------------ row stages
def _row_cases_by_form(gpu):
    by = {}
    for form, H, W, rho in R.row_cases(lambda rho: _taps(gpu, rho)):
        by.setdefault((form, rho), []).append((H, W))
    return by


def _row_ratio(gpu, form, H, W, rho, got=None):
    lam = R.library_tables(gpu, H)["lam"]
    b = R.row_input(H, W)
    ref = R.row_solve(b, rho, lam)
    got = _rows(gpu, b, rho, form) if got is None else got
    err = got - ref
    err = R.pair_error(err) if form == R.ROWS_DCT else np.abs(err)
    return float(np.max(err / R.row_bound(form, b, ref, rho, lam, _taps(gpu, rho))))


# (form, rho) with at least one admissible width: the Toeplitz kernels at the five small rhos -- the cooperative one
# without rho = 5, whose 95 terms are past its 64 -- the other two at all eight
FORCED = ([(R.ROWS_GREEN, r) for r in R.RHOS] + [(R.ROWS_COOP, r) for r in R.RHOS[:4]] +
          [(f, r) for f in (R.ROWS_DCT, R.ROWS_THOMAS) for r in R.RHOS + R.RHOS_LARGE])


@pytest.mark.parametrize("form,rho", FORCED)
def test_row_stage_forced(gpu, form, rho):
    """Each of the four row-stage kernels forced, at H = 8, 64 and the chirp heights 63, 65 (a 64-lane block with
    clamped lanes; DCT: even H only), at the widths where the kernel itself changes path -- COOP 384, 385, 767, 768, 769
    (one and two workgroups of 384 output columns, the mirror in the halo runs); GREEN 4t, 4t + 1, 127 .. 129, 511 ..
    513 where 4t allows (a wave's 128 and a workgroup's 512 columns), 384 and 513 at 65 <= t <= 96; DCT 8 .. 8192;
    THOMAS 1, 2, 15, 16, 17, 33, 255 (chunks of 16) -- for every rho of {1e-3, 0.3, 1, 2, 5} (THOMAS, DCT: also 300, 1e4,
    1e6) at which the form's precondition holds.  Reference: the long-double Thomas solve with the library's own lam
    table; bound: |err| <= c u inv(A)(|A||x| + |b|) element-wise with the derived c of tv2d_spectral_restated.py
    (C_THOMAS = 18 and the diagonal's formation, C_GREEN = 7 (t + 128) + 16, C_COOP = 744 and its rebuilt b; DCT
    norm-wise per row pair)."""
    by_form = _row_cases_by_form(gpu)
    assert set(by_form) == set(FORCED)  # (no admissible combination is left out, none is listed without a width)
    cases = by_form[(form, rho)]
    worst = 0.0
    for H, W in cases:
        ratio = _row_ratio(gpu, form, H, W, rho)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (form, H, W, rho, ratio)
    print(f"rows form={form} rho={rho}: {len(cases)} shapes, worst error/bound {worst:.4f}")


@pytest.mark.parametrize("H,W,rho", [(64, 384, 1.0), (64, 1024, 1.0), (63, 512, 0.3), (8, 1024, 2.0)])
def test_row_stage_forms_agree(gpu, H, W, rho):
    """all forms admissible at one shape agree within the sum of their bounds; AUTO returns the bits of the form
    admm_tv2d_row_stage names"""
    lam = R.library_tables(gpu, H)["lam"]
    b = R.row_input(H, W)
    ref = R.row_solve(b, rho, lam)
    t = _taps(gpu, rho)
    forms = [R.ROWS_GREEN, R.ROWS_COOP, R.ROWS_THOMAS] + ([R.ROWS_DCT] if R.is_pow2(W) and H % 2 == 0 else [])
    got = {f: _rows(gpu, b, rho, f) for f in forms}
    bound = {f: R.row_bound(f, b, ref, rho, lam, t) for f in forms}
    for i, f in enumerate(forms):
        for g in forms[i + 1:]:
            d = got[f] - got[g]
            if R.ROWS_DCT in (f, g):  # (the DCT bound is a norm over the row pair: the other form's bound as a norm too)
                other = f if g == R.ROWS_DCT else g
                assert np.all(R.pair_error(d) <= bound[R.ROWS_DCT] + R.pair_error(bound[other])), (f, g)
            else:
                assert np.all(np.abs(d) <= bound[f] + bound[g]), (f, g)
    named = gpu._lib.load().admm_tv2d_row_stage(H, W, rho)
    assert named in forms and np.array_equal(_rows(gpu, b, rho, R.ROWS_AUTO), got[named])


def test_auto_is_the_named_form_where_one_form_applies(gpu):
    for H, W, rho in [(64, 100, 1.0), (63, 64, 1.0), (64, 64, 1.0), (9, 1, 1.0), (64, 300, 10.0)]:
        named = gpu._lib.load().admm_tv2d_row_stage(H, W, rho)
        b = R.row_input(H, W)
        assert np.array_equal(_rows(gpu, b, rho, R.ROWS_AUTO), _rows(gpu, b, rho, named)), (H, W, rho)
        assert _row_ratio(gpu, named, H, W, rho) <= 1.0


# ------------------------------------------------------------------------------------------------ composed x-solve
@pytest.mark.parametrize("rho", R.XSOLVE_RHOS)
@pytest.mark.parametrize("H,W", R.XSOLVE_SHAPES)
def test_composed_xsolve(gpu, H, W, rho):
    """admm_op_tv2d_xsolve (forward columns, the row stage the rule names, inverse columns -- the function the loop
    calls) against the long-double composition with the library's lam table, in the Frobenius norm, inside the
    composition of the parts' bounds (xsolve_bound); at 8 x 8, 8 x 1 and 33 x 1 also against the dense long-double solve
    of (I + rho D'D) with D from np.diff, which has the EXACT eigenvalues where the composition has the table's (1 ulp,
    |d lam| <= 4u per direction; the inverse has norm <= 1): allowed as (1 + 8 rho) u ||x|| on top."""
    lam = R.library_tables(gpu, H)["lam"]
    b = R.xsolve_input(H, W)
    form = gpu._lib.load().admm_tv2d_row_stage(H, W, rho)
    ref, bh = R.xsolve(b, rho, lam)
    got = _rows(gpu, b, rho, R.ROWS_AUTO, xsolve=True)
    assert np.array_equal(got, _rows(gpu, b, rho, form, xsolve=True))
    fro = lambda a: np.sqrt(np.sum(np.asarray(a, dtype=LD) ** 2))
    bound = R.xsolve_bound(H, W, form, b, bh, ref, rho, lam, _taps(gpu, rho), R.hbr_max(gpu, H))
    ratio = float(fro(got - ref) / bound)
    print(f"xsolve {H}x{W} rho={rho} form={form}: error/bound {ratio:.4f}")
    assert ratio <= 1.0
    if (H, W) in R.XSOLVE_DENSE:
        dense = R.dense_xsolve(b, rho)
        assert float(fro(got - dense)) <= float(bound + (1 + 8 * rho) * R.U * fro(dense))


# ------------------------------------------------------------------------------------------------ errors
def test_bad_arguments_are_errors_not_launches(gpu):
    """H = 7, 8193, 5000 (the chirp form ends at 4096), W = 0, rho <= 0 or NaN, null pointers, and every forced form
    outside its own precondition: E_INVALID, and the output keeps its sentinel"""
    ops, (a, o) = R.spectral_op_calls(gpu)
    for name, kw in R.spectral_bad_calls():
        assert ops[name](**kw) == gpu._lib.E_INVALID, (name, kw)
    assert np.all(np.isnan(o))
    for name, call in ops.items():
        assert call() == gpu._lib.OK and not np.isnan(o[:64]).any() and np.all(np.isnan(o[64:])), name
        o[:] = np.nan
