"""The symmetric tile-packed product over a chunk of right-hand sides (symm.hip) through its operator
entry point admm_op_symm_packed, against the two references of test_gpu_ops_dense -- exact int64 arithmetic on integer
data, and the (n + 4) u |M||x| summation bound against a long-double product on normal data; no measured tolerance.
The operator builds the packed triangle from the lower triangle of M: everything above the diagonal is NaN here.

Orders: one tile with one and two rows, a tile short of / equal to / past 128, three tile rows with one live row in the
last, four and six tile rows.  K: one column, a whole chunk, and a second chunk with one and three live columns."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_ops_dense import IMAX, LD, U, _dp, _lower_storage, _ratio, _same_bits, _symv_case

pytestmark = pytest.mark.gpu

ORDERS = [1, 2, 127, 128, 129, 257, 385, 641]
KS = [1, 10, 11, 13]
MASKS = ("none", "first", "last", "every second", "all")


def _symm(gpu, M, n, Y, mask=None, X0=None):
    """X = M Y for the columns the mask leaves running; X starts as X0 (default: NaN, so a value nothing wrote shows)"""
    K = Y.shape[1]
    X = np.full((n, K), np.nan, order="F") if X0 is None else np.asfortranarray(X0.copy())
    Yf = np.asfortranarray(Y, dtype=np.float64)
    mp = None
    if mask is not None:
        mk = np.ascontiguousarray(mask, dtype=np.int32)
        mp = mk.ctypes.data_as(C.POINTER(C.c_int32))
    gpu._lib.check(gpu._lib.load().admm_op_symm_packed(_dp(gpu, M), n, M.shape[0], _dp(gpu, X), K, mp, _dp(gpu, Yf)))
    return X


@functools.lru_cache(maxsize=None)
def _case(n, K, kind):
    """(S, Y, ref, bound): S of test_gpu_ops_dense's case of this order, K right-hand sides of the same kind"""
    S = _symv_case(n, kind)[0]
    rng = np.random.default_rng(77 * n + K)
    if kind == "int":
        Y = rng.integers(-IMAX, IMAX + 1, (n, K))
        Si = S.astype(np.int64)
        assert np.max(np.abs(Si) @ np.abs(Y)) < 2 ** 53  # every partial sum is an integer fp64 holds
        return S, Y.astype(np.float64), (Si @ Y).astype(np.float64), None
    Y = rng.standard_normal((n, K))
    ref = S.astype(LD) @ Y.astype(LD)
    bound = (n + 4) * LD(U) * (np.abs(S).astype(LD) @ np.abs(Y).astype(LD))
    assert _ratio(S @ Y, ref, bound) <= 1.0  # NumPy's fp64 product obeys the bound
    return S, Y, ref, bound


def _mask(name, K):
    m = np.zeros(K, dtype=np.int32)
    if name == "first":
        m[0] = 1
    elif name == "last":
        m[-1] = 1
    elif name == "every second":
        m[::2] = 1
    elif name == "all":
        m[:] = 1
    return None if name == "none" else m


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", ORDERS)
def test_symm_exact(gpu, n, K):
    """integer data: bitwise the int64 product.  Catches the diagonal counted in both parts, a row or column of the last
    tile lost, a fit reading its neighbour's column of the interleaved layout, a chunk offset error"""
    S, Y, ref, _ = _case(n, K, "int")
    np.testing.assert_array_equal(_symm(gpu, _lower_storage(S), n, Y), ref)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", ORDERS)
def test_symm_bounded(gpu, n, K):
    """normal data inside the summation bound; a second call repeats the first bit for bit (fixed-order sums)"""
    S, Y, ref, bound = _case(n, K, "normal")
    M = _lower_storage(S)
    X = _symm(gpu, M, n, Y)
    worst = max(_ratio(X[:, k], ref[:, k], bound[:, k]) for k in range(K))
    print(f"symm n={n} K={K}: worst |err|/bound = {worst:.3f}")
    assert worst <= 1.0
    assert _same_bits(X, _symm(gpu, M, n, Y))


@pytest.mark.parametrize("K", [10, 13])
@pytest.mark.parametrize("n", [129, 257])
def test_symm_stop_mask(gpu, n, K):
    """a stopped fit keeps a NaN-free sentinel bit for bit; a running fit gives the bits it gives with no mask, whatever
    the other fits of its chunk do -- also when a stopped fit's right-hand side is NaN"""
    S, Y, _, _ = _case(n, K, "normal")
    M = _lower_storage(S)
    free = _symm(gpu, M, n, Y)
    X0 = np.asfortranarray(1e3 + np.arange(n * K, dtype=np.float64).reshape(n, K))
    for name in MASKS:
        mask = _mask(name, K)
        Yp = Y.copy()
        if mask is not None:
            Yp[:, mask != 0] = np.nan  # what a frozen fit leaves behind never reaches a running one
        X = _symm(gpu, M, n, Yp, mask, X0)
        for k in range(K):
            if mask is not None and mask[k]:
                assert _same_bits(X[:, k], X0[:, k]), f"mask {name}: stopped fit {k} was written"
            else:
                assert _same_bits(X[:, k], free[:, k]), f"mask {name}: running fit {k} changed its bits"


@pytest.mark.parametrize("fit", [0, 9, 10, 12])
@pytest.mark.parametrize("k", [0, 1, 63, 64, 127, 128, 129, 255, 256])
def test_symm_unit_vector_probe(gpu, k, fit):
    """M[r, j] = 1024 r + j (r >= j), Y = e_k in one fit and zero in the others: that fit's X is column k of the
    symmetrised M, so a wrong lane, quadrant, tile or fit shows as the index it was taken from; the others are zero"""
    n, K = 257, 13
    r, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    S = np.where(r >= j, 1024 * r + j, 1024 * j + r).astype(np.float64)
    Y = np.zeros((n, K))
    Y[k, fit] = 1.0
    want = np.zeros((n, K))
    want[:, fit] = S[:, k]
    np.testing.assert_array_equal(_symm(gpu, _lower_storage(S), n, Y), want)
