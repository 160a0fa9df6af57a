"""admm_op_softmax_prox on the GPU: the row prox of the multinomial loss alone, against the root of F in
np.longdouble (multinomial_restated.root_longdouble), measured as q49 defines it: ||F_longdouble(z)||_inf in
units of eps*max(1, ||v||_inf, a), under 10x the NumPy iteration's own worst figure (PROX_RATIO)."""
import ctypes as C

import numpy as np
import pytest

import multinomial_restated as R

pytestmark = pytest.mark.gpu

BOUND = 10.0 * R.PROX_RATIO


def softmax_prox(ap, V, y, a):
    lib = ap._lib.load()
    V = np.ascontiguousarray(V, dtype=np.float64)
    y32 = np.ascontiguousarray(y, dtype=np.int32)
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(V)
    iters = np.empty(V.shape[0], dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    ap._lib.check(lib.admm_op_softmax_prox(ap._lib.as_dp(V), y32.ctypes.data_as(ip), ap._lib.as_dp(a), V.shape[0],
                                           V.shape[1], ap._lib.as_dp(out), iters.ctypes.data_as(ip)))
    return out, iters


@pytest.mark.parametrize("m", R.PROX_ROWS)
@pytest.mark.parametrize("Cn", R.PROX_CLASSES)
def test_the_device_prox_meets_the_long_double_root(gpu, Cn, m):
    V, y, a = R.prox_inputs(Cn, m)
    Z, iters = softmax_prox(gpu, V, y, a)
    assert np.all(np.isfinite(Z))
    zero = a == 0.0
    assert zero.any() and np.array_equal(Z[zero].view(np.int64), V[zero].view(np.int64))  # a = 0: v bit for bit
    ratio = R.residual_ratio(Z, V, y, a)
    root = np.asarray(R.root_longdouble(V, y, a), dtype=np.float64)
    scale = np.maximum(np.maximum(1.0, a), np.abs(V).max(axis=1))
    dz = np.abs(Z - root).max(axis=1) / (R.EPS * scale)
    print(f"Cn {Cn} m {m}: residual ratio {ratio.max():.3f} (bound {BOUND}), |z - root| {dz.max():.3f} eps*scale, "
          f"Newton steps max {iters.max()} mean {iters.mean():.2f}")
    assert ratio.max() <= BOUND
    # the Jacobian is >= I, so ||z - root||_2 <= ||F(z)||_2 <= sqrt(Cn)*||F(z)||_inf
    assert dz.max() <= np.sqrt(Cn) * BOUND
    assert iters.max() < R.CAP and iters.min() >= 0
    assert np.all(iters[zero] == 0)


def test_bad_arguments_are_refused(gpu):
    V, y, a = R.prox_inputs(3, 33)
    with pytest.raises(gpu.AdmmError, match="no class"):
        softmax_prox(gpu, V, np.where(np.arange(33) == 4, 3, y), a)
    with pytest.raises(gpu.AdmmError, match=r"a\[2\]"):
        softmax_prox(gpu, V, y, np.where(np.arange(33) == 2, -1.0, a))
    with pytest.raises(gpu.AdmmError, match="Cn in 2"):
        softmax_prox(gpu, np.zeros((4, 11)), np.zeros(4), np.ones(4))
