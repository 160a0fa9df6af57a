"""The block soft threshold of the multi-fit lasso's grouped element kernel (csrc/group_multi.hip) through
admm_op_group_soft_threshold_multi: stage 2 of the prox alone, over the fit-interleaved layout and the kernel's own plan,
against grouplasso_restated.shrink in long double per fit.

Bound: penalty_restated.bound_ratio's, (p_g + 12)*eps*(|v_i| + t) per element with ratio <= 1 -- the rounding of a
p_g-term sum of squares, the root, the division, the subtraction and the product, relative to the sizes that enter."""
import ctypes as C

import numpy as np
import pytest

import grouplasso_restated as G
import penalty_restated as PR

pytestmark = pytest.mark.gpu

# n -> sizes: groups of one, groups that straddle 32-row blocks, a group above one block's budget and the last group
# ending at n; one group of 33; 31 groups of one; one group that a workgroup walks in 260 row blocks, twice
CASES = {700: PR.SIZES, 33: [33], 31: [1] * 31, 8300: [8300]}
KS = (1, 10, 11, 13)


def _op(gpu, V, sizes, t, weights=None, stop=None, Z=None):
    L = gpu._lib
    n, K = V.shape
    V = np.asfortranarray(V, dtype=np.float64)
    Z = np.full((n, K), np.nan, order="F") if Z is None else np.asfortranarray(Z, dtype=np.float64).copy(order="F")
    sz = np.ascontiguousarray(sizes, dtype=np.int64)
    t = np.ascontiguousarray(t, dtype=np.float64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    sm = None if stop is None else np.ascontiguousarray(stop, dtype=np.int32)
    L.check(L.load().admm_op_group_soft_threshold_multi(
        L.as_dp(V), n, K, sz.ctypes.data_as(C.POINTER(C.c_int64)), sz.size, None if w is None else L.as_dp(w), L.as_dp(t),
        None if sm is None else sm.ctypes.data_as(C.POINTER(C.c_int32)), L.as_dp(Z)))
    return Z


def _problem(n, K, sizes, seed):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((n, K)) * rng.uniform(0.2, 3.0, (1, K))
    w = rng.uniform(0.5, 2.0, len(sizes))
    norms = np.array([[np.linalg.norm(V[a:b, k]) for k in range(K)]
                      for a, b in zip(G.offsets(sizes)[:-1], G.offsets(sizes)[1:])])
    # per fit a threshold inside the range of its groups' norms / weights: some groups die, some live
    t = np.array([np.median(norms[:, k] / w) * (0.6 + 0.1 * (k % 5)) for k in range(K)])
    return V, w, t, norms


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", sorted(CASES))
def test_every_fit_matches_the_long_double_shrink(gpu, n, K):
    sizes = CASES[n]
    V, w, t, norms = _problem(n, K, sizes, seed=n + K)
    Z = _op(gpu, V, sizes, t, weights=w)
    again = _op(gpu, V, sizes, t, weights=w)
    assert np.array_equal(Z.view(np.uint64), again.view(np.uint64))  # two calls give equal bits
    worst = 0.0
    for k in range(K):
        exact = G.shrink(V[:, k], sizes, t[k], w, dtype=np.longdouble)
        worst = max(worst, PR.bound_ratio(V[:, k], Z[:, k], exact, PR.Penalty(sizes=sizes, groupweights=w), t[k]))
    print(f"n = {n}, K = {K}: worst error / bound {worst:.3f}")
    assert worst <= 1.0
    if len(sizes) > 1:  # the thresholds were placed so that both branches of the scale run
        dead = np.array([[np.all(Z[a:b, k] == 0.0) for k in range(K)]
                         for a, b in zip(G.offsets(sizes)[:-1], G.offsets(sizes)[1:])])
        assert dead.any() and not dead.all()


@pytest.mark.parametrize("n", sorted(CASES))
def test_zero_threshold_returns_v_and_a_large_one_exact_zeros(gpu, n):
    sizes = CASES[n]
    K = 11
    V, w, t, norms = _problem(n, K, sizes, seed=3 * n)
    t = t.copy()
    t[[0, 4, 10]] = 0.0                                    # bit for bit V
    big = 1.01 * float(np.max(norms / w[:, None]))
    t[[2, 9]] = big                                        # above every norm: exact zeros
    Z = _op(gpu, V, sizes, t, weights=w)
    for k in (0, 4, 10):
        assert np.array_equal(Z[:, k].view(np.uint64), np.ascontiguousarray(V[:, k]).view(np.uint64)), k
    for k in (2, 9):
        assert np.all(Z[:, k] == 0.0), k
    for k in (1, 3, 5, 6, 7, 8):  # the neighbours of the exact columns are what they are alone
        alone = _op(gpu, V[:, k:k + 1], sizes, t[k:k + 1], weights=w)
        assert np.array_equal(Z[:, k].view(np.uint64), alone[:, 0].view(np.uint64)), k


@pytest.mark.parametrize("n", (700, 8300))
def test_a_stopped_fit_keeps_its_column_and_changes_no_other(gpu, n):
    sizes = CASES[n]
    K = 13
    V, w, t, _ = _problem(n, K, sizes, seed=7 * n)
    Z0 = np.asfortranarray(np.random.default_rng(1).standard_normal((n, K)))
    stop = np.zeros(K, dtype=np.int32)
    stop[[3, 12]] = 1  # one in each chunk
    Z = _op(gpu, V, sizes, t, weights=w, stop=stop, Z=Z0)
    free = _op(gpu, V, sizes, t, weights=w)
    for k in range(K):
        want = Z0[:, k] if stop[k] else free[:, k]
        assert np.array_equal(Z[:, k].view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), k
    # a whole chunk stopped: its workgroups return before any load
    stop[:] = 0
    stop[10:] = 1
    Z = _op(gpu, V, sizes, t, weights=w, stop=stop, Z=Z0)
    assert np.array_equal(Z[:, 10:], Z0[:, 10:]) and np.array_equal(Z[:, :10], free[:, :10])


def test_refusals_name_the_culprit(gpu):
    L = gpu._lib
    lib = L.load()
    V = np.asfortranarray(np.ones((6, 2)))
    Z = np.asfortranarray(np.zeros((6, 2)))

    def call(sizes, w=None, t=(0.1, 0.1)):
        sz = np.ascontiguousarray(sizes, dtype=np.int64)
        tt = np.ascontiguousarray(t, dtype=np.float64)
        ww = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        rc = lib.admm_op_group_soft_threshold_multi(L.as_dp(V), 6, 2, sz.ctypes.data_as(C.POINTER(C.c_int64)), sz.size,
                                                    None if ww is None else L.as_dp(ww), L.as_dp(tt), None, L.as_dp(Z))
        return rc, lib.admm_last_error().decode()

    for args, part in ((dict(sizes=[3, 0, 3]), "group 1 has a size below 1"), (dict(sizes=[3, 2]), "sum to 5"),
                       (dict(sizes=[3, 3], w=[1.0, -1.0]), "weight 1"), (dict(sizes=[3, 3], t=(0.1, np.nan)), "t[1]")):
        rc, msg = call(**args)
        assert rc == L.E_INVALID and part in msg, (args, msg)
    assert np.all(Z == 0.0)  # a refused call writes nothing
