"""Host side of the width-selecting compact operator: admm_op_symv_compact_bits refuses bad arguments and every width
but 40 and 48 before it touches a device, and the storage getter refuses a NULL engine."""
import numpy as np


def test_operator_refuses_bad_arguments_and_widths_before_touching_a_device(ap):
    L = ap._lib
    lib, dp = L.load(), L.as_dp
    M, x, y = np.eye(4, order="F"), np.ones(4), np.zeros(4)
    for bits in (40, 48):
        assert lib.admm_op_symv_compact_bits(None, 4, 4, dp(x), 0, -1, 1, dp(y), None, 0, bits) == L.E_INVALID
        assert lib.admm_op_symv_compact_bits(dp(M), 4, 4, None, 0, -1, 1, dp(y), None, 0, bits) == L.E_INVALID
        assert lib.admm_op_symv_compact_bits(dp(M), 4, 4, dp(x), 0, -1, 1, None, None, 0, bits) == L.E_INVALID
        assert lib.admm_op_symv_compact_bits(dp(M), 0, 4, dp(x), 0, -1, 1, dp(y), None, 0, bits) == L.E_INVALID
        assert lib.admm_op_symv_compact_bits(dp(M), 4, 3, dp(x), 0, -1, 1, dp(y), None, 0, bits) == L.E_INVALID
        assert lib.admm_op_symv_compact_bits(dp(M), 4, 4, dp(x), 0, -2, 1, dp(y), None, 0, bits) == L.E_INVALID
        assert lib.admm_op_symv_compact_bits(dp(M), 4, 4, dp(x), 0, -1, 0, dp(y), None, 0, bits) == L.E_INVALID
        assert lib.admm_op_symv_compact_bits(dp(M), 4, 4, dp(x), 0, -1, 1, dp(y), dp(M), 3, bits) == L.E_INVALID
    for bits in (0, 39, 41, 47, 32, 64, -40):
        assert lib.admm_op_symv_compact_bits(dp(M), 4, 4, dp(x), 0, -1, 1, dp(y), None, 0, bits) == L.E_INVALID


def test_storage_getter_refuses_a_null_engine(ap):
    L = ap._lib
    assert L.load().admm_engine_xsolve_storage(None, None, None, None, None, None) == L.E_INVALID
    assert (L.STORAGE_FP64, L.STORAGE_COMPACT, L.STORAGE_COMPACT40) == (0, 1, 2)
