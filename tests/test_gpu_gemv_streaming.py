"""The forms of gemv_n_kernel / gemv_t_kernel (gemv.hip) that only large or very oblong matrices select: the
non-temporal-load instances (matrix above kStreamBytes) and, in gemv_t, the 4-deep main loop with its hand-over to the
tail loop and the odd row.  The shapes are those of test_gemv_forms_host.CASES, which pins on the host which form each
selects; every test here asks the planner again before it trusts its shape.

Exact references.  D holds integers in [-9, 9] and x / V integers in [-8, 8], so every product and every partial sum
is an integer below 72 * 2.1e6 < 2^53: every summation order, the device's and the host BLAS's, gives the same bits,
and the comparison is np.array_equal.  One dropped, doubled or misplaced element shows.  The floating-point case uses
the a-priori bound of a k-term sum in any order, |y - ref| <= gamma_k (|D| |x|), gamma_k = k u / (1 - k u), u = 2^-53,
k = the terms of an output plus the chunk partials summed behind them, against a reference in extended precision.

rows_per_chunk = 2048 with full chunks (four main-loop passes) needs 2048 column tiles of 2048+ rows (1 GB) or 4.2
million rows: left out, it adds passes and no region.  The one-chunk 449 x 65537 case runs the main loop under the
2048-row stride of the staged V."""
import ctypes as C
import math
import time

import numpy as np
import pytest

from test_gemv_forms_host import CASES, forms

pytestmark = pytest.mark.gpu


def _dp(ap, a):
    return ap._lib.as_dp(a)


def _gemv_n(ap, D, x):
    m, n = D.shape
    y = np.full(m, np.nan)
    ap._lib.check(ap._lib.load().admm_op_gemv_n(_dp(ap, D), m, n, m, _dp(ap, x), _dp(ap, y)))
    return y


def _gemv_t(ap, D, V):
    m, n = D.shape
    nrhs = V.shape[1]
    G = np.full((n, nrhs), np.nan, order="F")
    ap._lib.check(ap._lib.load().admm_op_gemv_t(_dp(ap, D), m, n, m, _dp(ap, V), m, nrhs, _dp(ap, G), n))
    return G


def _integer_case(m, n, rc):
    """column-major D (ld = m) of integers in [-4, 4] with other values planted where a clamp or an off-by-one would
    land: the last row, the last column, the first and the last row of the ragged last chunk; x and V in [-8, 8], not
    zero where they meet the planted entries"""
    rng = np.random.default_rng(m * 7 + n)
    D = rng.integers(-4, 5, size=(n, m), dtype=np.int8).astype(np.float64).T  # F-contiguous m x n
    assert D.flags["F_CONTIGUOUS"] and D.strides[1] == 8 * m
    r0 = (m - 1) // rc * rc  # first row of the last chunk
    j = np.arange(n)
    D[:, n - 1] = -(5 + np.arange(m) % 3)
    D[r0, :] = 8 + j % 2
    D[m - 1, :] = 5 + j % 3
    x = rng.integers(-8, 9, size=n).astype(np.float64)
    V = np.asfortranarray(rng.integers(-8, 9, size=(m, 3)).astype(np.float64))
    x[n - 1] = 7.0
    V[r0, :] = [-6.0, 4.0, 8.0]
    V[m - 1, :] = [7.0, -5.0, 3.0]
    return D, x, V


@pytest.mark.parametrize("m,n,rc,nt", CASES)
def test_gemv_large_forms_are_exact_on_integers(gpu, m, n, rc, nt):
    """gemv_n and gemv_t (nrhs = 3) on one matrix, bit for bit against D @ x and D' V, each call twice with the same
    bits (fixed-order sums); on the 256-row-chunk NT shape nrhs = 1 and 2 as well."""
    t0 = time.perf_counter()
    f = forms(gpu._lib, m, n)
    assert (f["t_rows_per_chunk"], f["nt"]) == (rc, nt), f
    D, x, V = _integer_case(m, n, rc)
    y_ref, G_ref = D @ x, D.T @ V
    assert np.all(y_ref == np.rint(y_ref)) and np.max(np.abs(G_ref)) < 2.0 ** 40
    t1 = time.perf_counter()
    y = _gemv_n(gpu, D, x)
    assert np.array_equal(y, y_ref), np.flatnonzero(y != y_ref)[:8]
    assert np.array_equal(_gemv_n(gpu, D, x), y)
    G = _gemv_t(gpu, D, V)
    assert np.array_equal(G, G_ref), np.argwhere(G != G_ref)[:8]
    assert np.array_equal(_gemv_t(gpu, D, V), G)
    if (rc, nt) == (256, 1):
        for nrhs in (1, 2):
            Vk = np.asfortranarray(V[:, 3 - nrhs:])  # (other columns than the leading ones)
            assert np.array_equal(_gemv_t(gpu, D, Vk), G_ref[:, 3 - nrhs:]), nrhs
    t2 = time.perf_counter()
    print(f"{m} x {n} {f}: host data and reference {t1 - t0:.2f} s, operator calls {t2 - t1:.2f} s")


def _extended(D, X, transpose):
    """(D X or D' X, |D| |X| or |D'| |X|) in extended precision by column blocks, or -- where long double is no wider
    than 60 bits -- by math.fsum on 64 sampled outputs; returns (indices, ref, mag)"""
    m, n = D.shape
    nout = n if transpose else m
    if np.finfo(np.longdouble).eps < 2.0 ** -60:
        ld = np.longdouble
        Xl = X.astype(ld)
        ref, mag = np.zeros((nout, X.shape[1]), dtype=ld), np.zeros((nout, X.shape[1]), dtype=ld)
        for j0 in range(0, n, 128):
            B = D[:, j0:j0 + 128].astype(ld)
            if transpose:
                ref[j0:j0 + 128], mag[j0:j0 + 128] = B.T @ Xl, np.abs(B).T @ np.abs(Xl)
            else:
                ref += B @ Xl[j0:j0 + 128]
                mag += np.abs(B) @ np.abs(Xl[j0:j0 + 128])
        return np.arange(nout), ref, mag
    idx = np.unique(np.linspace(0, nout - 1, 64).astype(np.int64))
    ref, mag = np.zeros((idx.size, X.shape[1])), np.zeros((idx.size, X.shape[1]))
    for a, i in enumerate(idx):
        d = D[:, i] if transpose else D[i, :]
        for c in range(X.shape[1]):
            ref[a, c], mag[a, c] = math.fsum(d * X[:, c]), math.fsum(np.abs(d * X[:, c]))  # (products: 1 ulp each)
    return idx, ref, mag


def test_gemv_nt_forms_within_the_a_priori_bound_on_normal_data(gpu):
    """standard-normal D, x and V at the smallest NT shape: per element within gamma_k (|D| |x|), k = n + column chunks
    for gemv_n and m + row chunks for gemv_t -- the bound of any summation order with fma, no measured constant"""
    m, n, rc, nt = CASES[0]
    f = forms(gpu._lib, m, n)
    assert (f["t_rows_per_chunk"], f["nt"]) == (rc, nt) == (256, 1), f
    rng = np.random.default_rng(20)
    D = np.asfortranarray(rng.standard_normal((n, m)).T)
    x = rng.standard_normal(n)
    V = np.asfortranarray(rng.standard_normal((m, 3)))
    u = 2.0 ** -53
    for name, got, (idx, ref, mag), k in (
            ("gemv_n", _gemv_n(gpu, D, x)[:, None], _extended(D, x[:, None], False), n + f["n_nchunk"]),
            ("gemv_t", _gemv_t(gpu, D, V), _extended(D, V, True), m + f["t_nchunk"])):
        gamma = k * u / (1.0 - k * u)
        err = np.abs(got[idx].astype(np.longdouble) - ref)
        ratio = float(np.max(err / (gamma * mag)))
        print(f"{name}: max |y - ref| / (gamma_{k} |D||x|) = {ratio:.3e}, max |y - ref| = {float(np.max(err)):.3e}")
        assert not np.isnan(got).any()
        assert np.all(err <= gamma * mag), (name, ratio)
