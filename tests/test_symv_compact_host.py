"""Host side of the compact x-solve storage: the acceptance rule create() applies to its probe, as the pure function of
the probe numbers the library exports (no device needed), and the argument checks of the operator entry."""
import math

import numpy as np


def test_acceptance_rule(ap):
    """keep compact while err_compact <= max(1e-11, 4 err_fp64) and diff <= max(1e-11, 8 err_fp64)"""
    ok = ap._lib.load().admm_xsolve_compact_accept
    assert ok(4e-15, 5e-15, 1e-14) == 1          # indistinguishable from fp64
    assert ok(9.9e-12, 1e-16, 9.9e-12) == 1      # under the floor whatever fp64 does
    assert ok(1e-11, 0.0, 1e-11) == 1            # the floor itself is inside
    assert ok(1.1e-11, 1e-13, 1e-13) == 0        # above the floor and above 4x
    assert ok(1e-13, 1e-13, 1.1e-11) == 0        # the second system decides too
    assert ok(3.9e-10, 1e-10, 7.9e-10) == 1      # a poor fp64 inverse widens both bounds: 4x and 8x
    assert ok(4.1e-10, 1e-10, 1e-12) == 0
    assert ok(1e-12, 1e-10, 8.1e-10) == 0
    for bad in ((math.nan, 1e-15, 1e-15), (1e-15, 1e-15, math.nan), (math.inf, 1e-15, 1e-15)):
        assert ok(*bad) == 0


def test_operator_refuses_bad_arguments_before_touching_a_device(ap):
    L = ap._lib
    lib, dp = L.load(), L.as_dp
    M, x, y = np.eye(4, order="F"), np.ones(4), np.zeros(4)
    assert lib.admm_op_symv_compact(None, 4, 4, dp(x), 0, -1, 1, dp(y), None, 0) == L.E_INVALID
    assert lib.admm_op_symv_compact(dp(M), 0, 4, dp(x), 0, -1, 1, dp(y), None, 0) == L.E_INVALID
    assert lib.admm_op_symv_compact(dp(M), 4, 3, dp(x), 0, -1, 1, dp(y), None, 0) == L.E_INVALID
    assert lib.admm_op_symv_compact(dp(M), 4, 4, dp(x), 0, -2, 1, dp(y), None, 0) == L.E_INVALID
    assert lib.admm_op_symv_compact(dp(M), 4, 4, dp(x), 0, -1, 0, dp(y), None, 0) == L.E_INVALID
    assert lib.admm_op_symv_compact(dp(M), 4, 4, dp(x), 0, -1, 1, dp(y), dp(M), 3) == L.E_INVALID
    assert lib.admm_engine_xsolve_storage(None, None, None, None, None, None) == L.E_INVALID
