"""ctypes binding of libadmm_hip.so (include/admm_engine.h).

The product path has no CPU fallback: if the shared library is missing or no HIP device
is visible, every compute entry point raises ``AdmmError`` loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libadmm_hip.so")

ABI_VERSION = 5

# error codes
OK, E_INVALID, E_UNSUPPORTED, E_DEVICE, E_NUMERIC, E_COMM, E_CAPACITY = 0, -1, -2, -3, -4, -5, -6

# problem kinds
PROB_LASSO, PROB_LASSO_CONSENSUS, PROB_LAD, PROB_HUBERFIT = 1, 2, 3, 4
PROB_LINEARSVM, PROB_TOTALVARIATION, PROB_QP_BOUNDED, PROB_BASISPURSUIT = 5, 6, 7, 8
PROB_MODEL, PROB_LINEARPROGRAM, PROB_QP_STANDARD, PROB_TV2D = 9, 10, 11, 12
PROB_COVSEL = 13
LOSS_HINGE, LOSS_01, LOSS_HINGE_OBJ01, LOSS_LOGISTIC = 0, 1, 2, 3
LOSS_SQHINGE = 5  # (4 is unassigned and refused)


def loss_code(text):
    """options.lossfunction -> ADMM_LOSS_*: 'hinge', '01' (as written), 'logistic'  and 'sqhinge'
     in any letter case; every other string runs the hinge prox with the 0-1 objective (linearsvm.m:154-158, 231-237: q18)."""
    if text in ("hinge", "01"):
        return LOSS_HINGE if text == "hinge" else LOSS_01
    if isinstance(text, str) and text.lower() == "logistic":
        return LOSS_LOGISTIC
    if isinstance(text, str) and text.lower() == "sqhinge":
        return LOSS_SQHINGE
    return LOSS_HINGE_OBJ01


XSOLVE_AUTO, XSOLVE_TRSV, XSOLVE_INVERSE, XSOLVE_CG, XSOLVE_CALLBACK, XSOLVE_PINV = 0, 1, 2, 3, 4, 5
MEM_HOST, MEM_DEVICE = 0, 1
STOP_STANDARD, STOP_HNORM, STOP_BOTH, STOP_NONE = 0, 1, 2, 3
FAST_OFF, FAST_STRONG, FAST_WEAK = 0, 1, 2

# fetch fields
(F_XOPT, F_ZOPT, F_UOPT, F_XVALS, F_ZVALS, F_UVALS, F_PNORM, F_DNORM, F_PERR, F_DERR, F_OBJEVALS, F_HNORMSQ,
 F_AVALS, F_DVALS, F_RESTARTED, F_VVALS, F_UHATVALS, F_ZCONSENSUS, F_FACTOR, F_CG_ITERS, F_CONS_X,
 F_CONS_U) = range(1, 23)

K_XSOLVE, K_GEMV_N, K_GEMV_T, K_PROX, K_FINALIZE, K_COUNT = 0, 1, 2, 3, 4, 5
COMM_ID_BYTES = 128
COMM_RCCL, COMM_SHM, COMM_P2P = 0, 1, 2

_dp = C.POINTER(C.c_double)


class ProblemDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("problem", C.c_int32),
        ("m", C.c_int64), ("n", C.c_int64),
        ("D", _dp), ("ldD", C.c_int64),
        ("s", _dp), ("ell", _dp), ("P", _dp), ("q", _dp), ("lb", _dp), ("ub", _dp), ("L", _dp),
        ("lambda_", C.c_double), ("C", C.c_double), ("r", C.c_double), ("rho", C.c_double),
        ("loss", C.c_int32), ("userelax", C.c_int32), ("xsolve", C.c_int32), ("mem", C.c_int32),
        ("device", C.c_int32), ("nslices", C.c_int32),
        ("slices", C.POINTER(C.c_int64)),
        ("comm", C.c_void_p),
        ("cg_tol", C.c_double), ("cg_maxit", C.c_int32), ("obj_gram", C.c_int32),
        ("Q", _dp), ("qz", _dp), ("D2", _dp), ("m2", C.c_int64), ("ldD2", C.c_int64), ("s2", _dp), ("c", _dp),
        ("K", _dp), ("k0", _dp), ("Dplus", _dp), ("Dts", _dp),
    ]


# caller-supplied prox operators / objective (device pointers as integers; see admm_engine.h)
PROX_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                            C.c_int64, C.c_void_p)
OPERATOR_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p)
OBJ_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)
ALTU_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                            C.c_void_p)
NORMS_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                             C.c_double, C.c_void_p, C.c_void_p)


class Options(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("maxiters", C.c_int32),
        ("rho", C.c_double), ("relax", C.c_double), ("abstol", C.c_double), ("reltol", C.c_double),
        ("Hnormtol", C.c_double), ("convtol", C.c_double), ("restart", C.c_double), ("dvaltol", C.c_double),
        ("domaxiters", C.c_int32), ("fast", C.c_int32), ("objevals", C.c_int32), ("convtest", C.c_int32),
        ("stopcond", C.c_int32), ("nodualerror", C.c_int32), ("record_history", C.c_int32),
        ("check_every", C.c_int32),
        ("x0", _dp), ("z0", _dp), ("u0", _dp),
        ("stale_factor_ok", C.c_int32), ("reserved1", C.c_int32),
    ]


class RunSummary(C.Structure):
    _fields_ = [
        ("steps", C.c_int32), ("stopped_early", C.c_int32), ("convtest_failed_at", C.c_int32),
        ("obj_gram_used", C.c_int32), ("runtime_s", C.c_double), ("objopt", C.c_double),
    ]


class PenaltyDesc(C.Structure):  # admm_penalty_desc
    _fields_ = [("l1weights", C.POINTER(C.c_double)), ("l1", C.c_double), ("ridge", C.c_double),
                ("nonnegative", C.c_int32)]


class LossDesc(C.Structure):  # admm_loss_desc
    _fields_ = [("weights", C.POINTER(C.c_double)), ("slope_pos", C.c_double), ("slope_neg", C.c_double),
                ("epsilon", C.c_double), ("delta", C.c_double)]


class SvmCostDesc(C.Structure):  # admm_svm_cost_desc
    _fields_ = [("weights", C.POINTER(C.c_double)), ("cost_pos", C.c_double), ("cost_neg", C.c_double)]


class SparseDesc(C.Structure):  # admm_sparse_desc: real double CSC
    _fields_ = [("struct_size", C.c_int32), ("mem", C.c_int32), ("rows", C.c_int64), ("cols", C.c_int64),
                ("nnz", C.c_int64), ("val", C.POINTER(C.c_double)), ("ir", C.POINTER(C.c_uint64)),
                ("jc", C.POINTER(C.c_uint64))]


def canonical_csc(D):
    """any scipy.sparse matrix or array -> (rows, cols, val float64, ir uint64, jc uint64) in canonical CSC: duplicates
    summed, row indices ascending inside a column -- what admm_engine_create_sparse accepts"""
    import numpy as np
    import scipy.sparse as sp

    if not sp.issparse(D):
        raise TypeError("not a scipy.sparse matrix")
    A = sp.csc_matrix(D, dtype=np.float64, copy=True)  # (a copy: the caller's matrix is never reordered in place)
    A.sum_duplicates()
    A.sort_indices()
    rows, cols = A.shape
    return (int(rows), int(cols), np.ascontiguousarray(A.data, dtype=np.float64),
            np.ascontiguousarray(A.indices, dtype=np.uint64), np.ascontiguousarray(A.indptr, dtype=np.uint64))


def sparse_desc(D, keep):
    """admm_sparse_desc of a scipy.sparse matrix over host arrays appended to ``keep``"""
    rows, cols, val, ir, jc = canonical_csc(D)
    keep.extend((val, ir, jc))
    d = SparseDesc()
    d.struct_size = C.sizeof(SparseDesc)
    d.mem = MEM_HOST
    d.rows, d.cols, d.nnz = rows, cols, int(val.size)
    d.val = val.ctypes.data_as(C.POINTER(C.c_double))
    d.ir = ir.ctypes.data_as(C.POINTER(C.c_uint64))
    d.jc = jc.ctypes.data_as(C.POINTER(C.c_uint64))
    return d


def is_sparse(D):
    """True for a scipy.sparse matrix or array (scipy is imported only when D is not a NumPy array)"""
    if D is None or isinstance(D, (list, tuple)) or type(D).__module__.startswith("numpy"):
        return False
    try:
        import scipy.sparse as sp
    except ImportError:
        return False
    return sp.issparse(D)


class EngineInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("xsolve_requested", C.c_int32), ("xsolve_used", C.c_int32),
        ("pinv_used", C.c_int32), ("probed", C.c_int32), ("trsv_blocks", C.c_int32), ("jacobi_sweeps", C.c_int32),
        ("unwrapped_fused", C.c_int32), ("factor_n", C.c_int64), ("rank", C.c_int64),
        ("cond_estimate", C.c_double), ("probe_err_inverse", C.c_double), ("probe_err_trsv", C.c_double),
        ("probe_diff", C.c_double), ("xsolve_cacheable_bytes", C.c_int64), ("xsolve_stream_bytes", C.c_int64),
        ("obj_bound_max", C.c_double), ("obj_form_literal", C.c_int32), ("ngroups", C.c_int32),
        ("probe_err_trsv_one", C.c_double),
    ]


class Field(C.Structure):  # admm_field: one field of a host struct as the binding layer reads it
    _fields_ = [("name", C.c_char_p), ("kind", C.c_int32), ("reserved", C.c_int32), ("data", C.POINTER(C.c_double)),
                ("rows", C.c_int64), ("cols", C.c_int64), ("text", C.c_char_p), ("ir", C.POINTER(C.c_uint64)),
                ("jc", C.POINTER(C.c_uint64))]


class BindingInfo(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("problem", C.c_int32), ("nA", C.c_int64), ("nB", C.c_int64),
                ("nU", C.c_int64), ("a_handle", C.c_int32), ("b_kind", C.c_int32), ("b_scalar", C.c_double),
                ("b_matrix", C.POINTER(C.c_double)), ("b_ld", C.c_int64)]


class ResultField(C.Structure):
    _fields_ = [("name", C.c_char_p), ("kind", C.c_int32), ("source", C.c_int32), ("rows", C.c_int64),
                ("cols", C.c_int64), ("scalar", C.c_double)]


class SvmOvrDesc(C.Structure):  # admm_svm_ovr_desc
    _fields_ = [("struct_size", C.c_int32), ("K", C.c_int32), ("m", C.c_int64), ("n", C.c_int64), ("D", _dp),
                ("ldD", C.c_int64), ("ELL", _dp), ("loss", C.POINTER(C.c_int32)), ("C", C.c_double),
                ("mem", C.c_int32), ("device", C.c_int32), ("Dplus", _dp), ("comm", C.c_void_p)]


class SvmOvrOptions(C.Structure):  # admm_svm_ovr_options
    _fields_ = [("struct_size", C.c_int32), ("maxiters", C.c_int32), ("rho", C.c_double), ("abstol", C.c_double),
                ("reltol", C.c_double), ("Hnormtol", C.c_double), ("relax", C.c_double), ("fast", C.c_int32),
                ("convtest", C.c_int32), ("domaxiters", C.c_int32), ("objevals", C.c_int32),
                ("check_every", C.c_int32), ("reserved0", C.c_int32), ("x0", _dp), ("z0", _dp), ("u0", _dp)]


class SvmOvrSummary(C.Structure):  # admm_svm_ovr_summary
    _fields_ = [("steps", C.c_int32), ("stopped_early", C.c_int32), ("objopt", C.c_double)]


OVR_F_XOPT, OVR_F_ZOPT, OVR_F_UOPT, OVR_F_PNORM, OVR_F_PERR, OVR_F_HNORMSQ, OVR_F_OBJEVALS = range(1, 8)
SVM_OVR_MAX_N = 448


class RegMultiDesc(C.Structure):  # admm_reg_multi_desc
    _fields_ = [("struct_size", C.c_int32), ("K", C.c_int32), ("m", C.c_int64), ("n", C.c_int64), ("D", _dp),
                ("ldD", C.c_int64), ("S", _dp), ("ns", C.c_int32), ("mem", C.c_int32), ("device", C.c_int32),
                ("reserved0", C.c_int32), ("kind", C.POINTER(C.c_int32)), ("a", _dp), ("b", _dp), ("epsilon", _dp),
                ("delta", _dp), ("comm", C.c_void_p)]


class RegMultiOptions(C.Structure):  # admm_reg_multi_options
    _fields_ = [("struct_size", C.c_int32), ("maxiters", C.c_int32), ("rho", C.c_double), ("abstol", C.c_double),
                ("reltol", C.c_double), ("relax", C.c_double), ("fast", C.c_int32), ("convtest", C.c_int32),
                ("domaxiters", C.c_int32), ("objevals", C.c_int32), ("check_every", C.c_int32),
                ("reserved0", C.c_int32), ("x0", _dp), ("z0", _dp), ("u0", _dp)]


class RegMultiSummary(C.Structure):  # admm_reg_multi_summary
    _fields_ = [("steps", C.c_int32), ("stopped_early", C.c_int32), ("objopt", C.c_double)]


REGM_F_XOPT, REGM_F_ZOPT, REGM_F_UOPT, REGM_F_PNORM, REGM_F_PERR, REGM_F_OBJEVALS = range(1, 7)
REG_MULTI_MAX_N = 448
REGM_KIND_LAD, REGM_KIND_HUBER = 0, 1

class SparseSvmDesc(C.Structure):  # admm_sparse_svm_desc
    _fields_ = [("struct_size", C.c_int32), ("K", C.c_int32), ("D", C.POINTER(SparseDesc)), ("ELL", _dp),
                ("loss", C.POINTER(C.c_int32)), ("C", C.c_double), ("device", C.c_int32), ("reserved0", C.c_int32),
                ("comm", C.c_void_p)]


class SparseSvmOptions(C.Structure):  # admm_sparse_svm_options
    _fields_ = [("struct_size", C.c_int32), ("maxiters", C.c_int32), ("rho", C.c_double), ("abstol", C.c_double),
                ("reltol", C.c_double), ("Hnormtol", C.c_double), ("relax", C.c_double), ("fast", C.c_int32),
                ("convtest", C.c_int32), ("domaxiters", C.c_int32), ("objevals", C.c_int32),
                ("check_every", C.c_int32), ("cg_maxit", C.c_int32), ("cg_tol", C.c_double), ("x0", _dp), ("z0", _dp),
                ("u0", _dp)]


class SparseSvmSummary(C.Structure):  # admm_sparse_svm_summary
    _fields_ = [("steps", C.c_int32), ("stopped_early", C.c_int32), ("objopt", C.c_double),
                ("cg_iters_total", C.c_int64), ("cg_capped_updates", C.c_int64)]


class SparseRegDesc(C.Structure):  # admm_sparse_reg_desc
    _fields_ = [("struct_size", C.c_int32), ("K", C.c_int32), ("D", C.POINTER(SparseDesc)), ("S", _dp),
                ("ns", C.c_int32), ("device", C.c_int32), ("kind", C.POINTER(C.c_int32)), ("a", _dp), ("b", _dp),
                ("epsilon", _dp), ("delta", _dp), ("comm", C.c_void_p)]


class SparseRegOptions(C.Structure):  # admm_sparse_reg_options
    _fields_ = [("struct_size", C.c_int32), ("maxiters", C.c_int32), ("rho", C.c_double), ("abstol", C.c_double),
                ("reltol", C.c_double), ("relax", C.c_double), ("fast", C.c_int32), ("convtest", C.c_int32),
                ("domaxiters", C.c_int32), ("objevals", C.c_int32), ("check_every", C.c_int32),
                ("cg_maxit", C.c_int32), ("cg_tol", C.c_double), ("nodualerror", C.c_int32), ("reserved0", C.c_int32),
                ("x0", _dp), ("z0", _dp), ("u0", _dp)]


class SparseRegSummary(C.Structure):  # admm_sparse_reg_summary
    _fields_ = [("steps", C.c_int32), ("stopped_early", C.c_int32), ("objopt", C.c_double),
                ("cg_iters_total", C.c_int64), ("cg_capped_updates", C.c_int64)]


(SRG_F_XOPT, SRG_F_ZOPT, SRG_F_UOPT, SRG_F_PNORM, SRG_F_PERR, SRG_F_OBJEVALS, SRG_F_DNORM,
 SRG_F_DERR) = range(1, 9)


class SparseLassoDesc(C.Structure):  # admm_sparse_lasso_desc
    _fields_ = [("struct_size", C.c_int32), ("K", C.c_int32), ("D", C.POINTER(SparseDesc)), ("S", _dp),
                ("ns", C.c_int32), ("device", C.c_int32), ("lam", _dp), ("ridge", _dp),
                ("nonneg", C.POINTER(C.c_int32)), ("weights", _dp), ("comm", C.c_void_p)]


class SparseLassoOptions(C.Structure):  # admm_sparse_lasso_options
    _fields_ = list(SparseRegOptions._fields_)


class SparseLassoSummary(C.Structure):  # admm_sparse_lasso_summary
    _fields_ = list(SparseRegSummary._fields_)


(SLM_F_XOPT, SLM_F_ZOPT, SLM_F_UOPT, SLM_F_PNORM, SLM_F_PERR, SLM_F_OBJEVALS, SLM_F_DNORM,
 SLM_F_DERR) = range(1, 9)


class LassoMultiDesc(C.Structure):  # admm_lasso_multi_desc
    _fields_ = [("struct_size", C.c_int32), ("K", C.c_int32), ("m", C.c_int64), ("n", C.c_int64), ("D", _dp),
                ("ldD", C.c_int64), ("S", _dp), ("ns", C.c_int32), ("device", C.c_int32), ("rho", C.c_double),
                ("xsolve", C.c_int32), ("reserved0", C.c_int32), ("lam", _dp), ("ridge", _dp),
                ("nonneg", C.POINTER(C.c_int32)), ("weights", _dp), ("comm", C.c_void_p)]


class LassoMultiOptions(C.Structure):  # admm_lasso_multi_options
    _fields_ = [("struct_size", C.c_int32), ("maxiters", C.c_int32), ("rho", C.c_double), ("abstol", C.c_double),
                ("reltol", C.c_double), ("relax", C.c_double), ("fast", C.c_int32), ("convtest", C.c_int32),
                ("domaxiters", C.c_int32), ("objevals", C.c_int32), ("check_every", C.c_int32),
                ("nodualerror", C.c_int32), ("x0", _dp), ("z0", _dp), ("u0", _dp)]


class LassoMultiSummary(C.Structure):  # admm_lasso_multi_summary
    _fields_ = [("steps", C.c_int32), ("stopped_early", C.c_int32), ("objopt", C.c_double), ("xsolve", C.c_int32),
                ("reserved0", C.c_int32)]


(LM_F_XOPT, LM_F_ZOPT, LM_F_UOPT, LM_F_PNORM, LM_F_PERR, LM_F_OBJEVALS, LM_F_DNORM, LM_F_DERR) = range(1, 9)


class CovselMultiDesc(C.Structure):  # admm_covsel_multi_desc
    _fields_ = [("struct_size", C.c_int32), ("K", C.c_int32), ("m", C.c_int64), ("n", C.c_int64), ("D", _dp),
                ("ldD", C.c_int64), ("S", _dp), ("lam", _dp), ("device", C.c_int32), ("reserved0", C.c_int32),
                ("comm", C.c_void_p)]


class CovselMultiOptions(C.Structure):  # admm_covsel_multi_options
    _fields_ = [("struct_size", C.c_int32), ("maxiters", C.c_int32), ("rho", C.c_double), ("abstol", C.c_double),
                ("reltol", C.c_double), ("relax", C.c_double), ("fast", C.c_int32), ("convtest", C.c_int32),
                ("domaxiters", C.c_int32), ("objevals", C.c_int32), ("check_every", C.c_int32),
                ("nodualerror", C.c_int32), ("rhos", _dp), ("z0", _dp), ("u0", _dp)]


class CovselMultiSummary(C.Structure):  # admm_covsel_multi_summary
    _fields_ = [("steps", C.c_int32), ("stopped_early", C.c_int32), ("objopt", C.c_double),
                ("jacobi_sweeps", C.c_int32), ("reserved0", C.c_int32)]


(CM_F_XOPT, CM_F_ZOPT, CM_F_UOPT, CM_F_PNORM, CM_F_PERR, CM_F_OBJEVALS, CM_F_DNORM, CM_F_DERR, CM_F_COV) = range(1, 10)
COVSEL_SMALL_MAX = 96  # csrc/covsel.h: kCovselSmallMax, the largest n of a fit that stays in one workgroup's LDS


class L1ClassDesc(C.Structure):  # admm_l1class_desc
    _fields_ = [("struct_size", C.c_int32), ("K", C.c_int32), ("m", C.c_int64), ("n", C.c_int64), ("D", _dp),
                ("ldD", C.c_int64), ("ELL", _dp), ("nell", C.c_int32), ("device", C.c_int32), ("C", C.c_double),
                ("xsolve", C.c_int32), ("reserved0", C.c_int32), ("loss", C.POINTER(C.c_int32)), ("lam", _dp),
                ("ridge", _dp), ("nonneg", C.POINTER(C.c_int32)), ("l1weights", _dp), ("comm", C.c_void_p)]


class L1ClassOptions(C.Structure):  # admm_l1class_options
    _fields_ = list(LassoMultiOptions._fields_)


class L1ClassSummary(C.Structure):  # admm_l1class_summary
    _fields_ = list(LassoMultiSummary._fields_)


(L1C_F_XOPT, L1C_F_ZOPT, L1C_F_UOPT, L1C_F_PNORM, L1C_F_PERR, L1C_F_OBJEVALS, L1C_F_DNORM, L1C_F_DERR) = range(1, 9)


class SparseL1ClassDesc(C.Structure):  # admm_sparse_l1class_desc
    _fields_ = [("struct_size", C.c_int32), ("K", C.c_int32), ("D", C.POINTER(SparseDesc)), ("ELL", _dp),
                ("nell", C.c_int32), ("device", C.c_int32), ("C", C.c_double), ("xsolve", C.c_int32),
                ("reserved0", C.c_int32), ("loss", C.POINTER(C.c_int32)), ("lam", _dp), ("ridge", _dp),
                ("nonneg", C.POINTER(C.c_int32)), ("l1weights", _dp), ("comm", C.c_void_p)]


class SparseL1ClassOptions(C.Structure):  # admm_sparse_l1class_options
    _fields_ = list(SparseRegOptions._fields_)


class SparseL1ClassSummary(C.Structure):  # admm_sparse_l1class_summary (admm_sparse_l1class_fetch: the L1C_F_* fields)
    _fields_ = [("steps", C.c_int32), ("stopped_early", C.c_int32), ("objopt", C.c_double), ("xsolve", C.c_int32),
                ("reserved0", C.c_int32), ("cg_iters_total", C.c_int64), ("cg_capped_updates", C.c_int64)]


FIELD_NUMERIC, FIELD_TEXT, FIELD_HANDLE, FIELD_SPARSE, FIELD_OTHER = 0, 1, 2, 3, 4
RES_FETCH, RES_SCALAR, RES_START = 0, 1, 2
STORAGE_FP64, STORAGE_COMPACT, STORAGE_COMPACT40, STORAGE_COMPACT38, STORAGE_COMPACT36 = 0, 1, 2, 3, 4
F_WVALS = 23
F_COVSEL_S = 24
F_TV2D_ROW_STAGE = 25
F_SPARSE_NNZ = 26
TV2D_ROWS_AUTO, TV2D_ROWS_GREEN, TV2D_ROWS_COOP, TV2D_ROWS_DCT, TV2D_ROWS_THOMAS = range(5)
TV2D_ROWS_NAMES = ("cg", "green", "coop", "dct", "thomas")  # results["tv2d_row_stage"] (0: no spectral x-update)


class AdmmError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"[admm_hip {code}] {message}")
        self.code = code


# every symbol include/admm_engine.h declares, with its signature
_SIGNATURES = {
    "admm_abi_version": (C.c_int, []),
    "admm_last_error": (C.c_char_p, []),
    "admm_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "admm_device_info": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "admm_options_default": (None, [C.POINTER(Options)]),
    "admm_problem_desc_default": (None, [C.POINTER(ProblemDesc)]),
    "admm_engine_create": (C.c_int, [C.POINTER(ProblemDesc), C.POINTER(C.c_void_p)]),
    "admm_engine_create_sparse": (C.c_int, [C.POINTER(ProblemDesc), C.POINTER(SparseDesc), C.POINTER(C.c_void_p)]),
    "admm_engine_set_callbacks": (C.c_int, [C.c_void_p, PROX_CALLBACK, C.c_void_p, PROX_CALLBACK, C.c_void_p,
                                            OBJ_CALLBACK, C.c_void_p]),
    "admm_engine_set_operators": (C.c_int, [C.c_void_p, OPERATOR_CALLBACK, C.c_void_p, OPERATOR_CALLBACK, C.c_void_p]),
    "admm_engine_set_constraint_b": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int64, C.c_int64, C.c_int32,
                                               C.c_double, OPERATOR_CALLBACK, C.c_void_p]),
    "admm_engine_set_groups": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int32, _dp]),
    "admm_engine_set_penalty": (C.c_int, [C.c_void_p, C.POINTER(PenaltyDesc)]),
    "admm_engine_get_penalty": (C.c_int, [C.c_void_p, C.POINTER(PenaltyDesc), C.POINTER(C.c_int32)]),
    "admm_engine_set_loss": (C.c_int, [C.c_void_p, C.POINTER(LossDesc)]),
    "admm_engine_get_loss": (C.c_int, [C.c_void_p, C.POINTER(LossDesc), C.POINTER(C.c_int32)]),
    "admm_engine_set_svm_cost": (C.c_int, [C.c_void_p, C.POINTER(SvmCostDesc)]),
    "admm_engine_get_svm_cost": (C.c_int, [C.c_void_p, C.POINTER(SvmCostDesc), C.POINTER(C.c_int32)]),
    "admm_engine_set_tv2d_isotropic": (C.c_int, [C.c_void_p, C.c_int32]),
    "admm_engine_run": (C.c_int, [C.c_void_p, C.POINTER(Options), C.POINTER(RunSummary)]),
    "admm_engine_fetch": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "admm_engine_set_hooks": (C.c_int, [C.c_void_p, ALTU_CALLBACK, C.c_void_p, NORMS_CALLBACK, C.c_void_p]),
    "admm_engine_info": (C.c_int, [C.c_void_p, C.POINTER(EngineInfo)]),
    "admm_engine_xsolve_storage": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                             C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "admm_xsolve_compact_accept": (C.c_int, [C.c_double, C.c_double, C.c_double]),
    "admm_engine_xsolve_rejected": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, _dp,
                                              _dp]),
    "admm_symv_compact_tile_offset": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]),
    "admm_tv2d_row_stage": (C.c_int, [C.c_int64, C.c_int64, C.c_double]),
    "admm_tv2d_rows_green_taps": (C.c_int, [C.c_double]),
    "admm_dct_tables": (C.c_int, [C.c_int64, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_int64)]),
    "admm_engine_setup_seconds": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "admm_engine_kernel_time": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "admm_engine_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "admm_engine_set_profiling_stride": (C.c_int, [C.c_void_p, C.c_int]),
    "admm_engine_destroy": (None, [C.c_void_p]),
    "admm_binding_create": (C.c_int, [C.c_char_p, C.POINTER(Field), C.c_int32, C.POINTER(Field), C.c_int32,
                                      C.POINTER(C.c_void_p)]),
    "admm_binding_destroy": (None, [C.c_void_p]),
    "admm_binding_desc": (C.POINTER(ProblemDesc), [C.c_void_p]),
    "admm_binding_sparse": (C.POINTER(SparseDesc), [C.c_void_p]),
    "admm_binding_get_info": (C.c_int, [C.c_void_p, C.POINTER(BindingInfo)]),
    "admm_binding_apply": (C.c_int, [C.c_void_p, C.c_void_p]),
    "admm_binding_options": (C.c_int, [C.c_void_p, C.POINTER(Field), C.c_int32, C.POINTER(Field), C.c_int32,
                                       C.POINTER(Options)]),
    "admm_binding_results": (C.c_int, [C.c_void_p, C.POINTER(Options), C.POINTER(RunSummary), C.POINTER(ResultField),
                                       C.c_int32, C.POINTER(C.c_int32)]),
    "admm_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "admm_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "admm_op_gemv_n": (C.c_int, [_dp, C.c_int64, C.c_int64, C.c_int64, _dp, _dp]),
    "admm_op_gemv_t": (C.c_int, [_dp, C.c_int64, C.c_int64, C.c_int64, _dp, C.c_int64, C.c_int32, _dp, C.c_int64]),
    "admm_op_gemv_forms": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int32)]),
    "admm_op_spmv": (C.c_int, [C.POINTER(SparseDesc), C.c_int, _dp, _dp]),
    "admm_op_gram": (C.c_int, [_dp, C.c_int64, C.c_int64, C.c_int64, C.c_double, _dp]),
    "admm_op_cholesky": (C.c_int, [_dp, C.c_int64, C.c_int64]),
    "admm_op_trsv_pair": (C.c_int, [_dp, C.c_int64, C.c_int64, _dp, _dp]),
    "admm_op_soft_threshold": (C.c_int, [_dp, C.c_int64, C.c_double, _dp]),
    "admm_op_pair_soft_threshold": (C.c_int, [_dp, C.c_int64, C.c_double, _dp]),
    "admm_op_group_soft_threshold": (C.c_int, [_dp, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _dp, C.c_double, _dp]),
    "admm_op_penalty_prox": (C.c_int, [_dp, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _dp, C.c_double,
                                       C.POINTER(PenaltyDesc), C.c_double, _dp]),
    "admm_op_loss_prox": (C.c_int, [_dp, C.c_int64, C.c_int32, C.POINTER(LossDesc), C.c_double, _dp]),
    "admm_op_svm_prox": (C.c_int, [_dp, _dp, C.c_int64, C.c_int32, C.c_double, C.c_double, C.POINTER(SvmCostDesc), _dp]),
    "admm_op_symv": (C.c_int, [_dp, C.c_int64, C.c_int64, _dp, C.c_int32, C.c_int64, C.c_int32, _dp]),
    "admm_op_symv_compact": (C.c_int, [_dp, C.c_int64, C.c_int64, _dp, C.c_int32, C.c_int64, C.c_int32, _dp, _dp,
                                       C.c_int64]),
    "admm_op_symv_compact_bits": (C.c_int, [_dp, C.c_int64, C.c_int64, _dp, C.c_int32, C.c_int64, C.c_int32, _dp, _dp,
                                            C.c_int64, C.c_int32]),
    "admm_op_symv_batch": (C.c_int, [_dp, C.c_int64, C.c_int64, C.c_int32, _dp, C.c_int64, C.c_int64, _dp, C.c_int64]),
    "admm_op_gemm": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_double, _dp, C.c_int64, _dp,
                               C.c_int64, C.c_double, _dp, C.c_int64, C.c_int32]),
    "admm_op_trtri": (C.c_int, [_dp, C.c_int64, C.c_int64, _dp, C.c_int64]),
    "admm_op_llt_apply": (C.c_int, [_dp, C.c_int64, C.c_int64, _dp, _dp]),
    "admm_op_dct_cols": (C.c_int, [_dp, C.c_int64, C.c_int64, C.c_int32, _dp]),
    "admm_op_tv2d_rows": (C.c_int, [_dp, C.c_int64, C.c_int64, C.c_double, C.c_int32, _dp]),
    "admm_op_tv2d_xsolve": (C.c_int, [_dp, C.c_int64, C.c_int64, C.c_double, C.c_int32, _dp]),
    "admm_op_consensus_tail": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double, _dp, _dp,
                                         _dp, _dp, _dp, _dp, _dp, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp]),
    "admm_comm_unique_id": (C.c_int, [C.c_char_p]),
    "admm_comm_init": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "admm_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "admm_comm_allreduce_sum": (C.c_int, [C.c_void_p, _dp, C.c_size_t]),
    "admm_comm_measure_latency": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    "admm_comm_destroy": (None, [C.c_void_p]),
    "admm_comm_init_all": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "admm_engine_create_all": (C.c_int, [C.c_int, C.POINTER(ProblemDesc), C.POINTER(C.c_void_p)]),
    "admm_engine_run_all": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(Options), C.c_int,
                                      C.POINTER(RunSummary)]),
    "admm_svm_ovr_desc_default": (None, [C.POINTER(SvmOvrDesc)]),
    "admm_svm_ovr_options_default": (None, [C.POINTER(SvmOvrOptions)]),
    "admm_svm_ovr_create": (C.c_int, [C.POINTER(SvmOvrDesc), C.POINTER(C.c_void_p)]),
    "admm_svm_ovr_run": (C.c_int, [C.c_void_p, C.POINTER(SvmOvrOptions), C.POINTER(SvmOvrSummary),
                                   C.POINTER(C.c_double)]),
    "admm_svm_ovr_fetch": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "admm_svm_ovr_set_cost": (C.c_int, [C.c_void_p, _dp, _dp]),
    "admm_svm_ovr_chunk": (C.c_int, []),
    "admm_svm_ovr_destroy": (None, [C.c_void_p]),
    "admm_reg_multi_desc_default": (None, [C.POINTER(RegMultiDesc)]),
    "admm_reg_multi_options_default": (None, [C.POINTER(RegMultiOptions)]),
    "admm_reg_multi_create": (C.c_int, [C.POINTER(RegMultiDesc), C.POINTER(C.c_void_p)]),
    "admm_reg_multi_run": (C.c_int, [C.c_void_p, C.POINTER(RegMultiOptions), C.POINTER(RegMultiSummary),
                                     C.POINTER(C.c_double)]),
    "admm_reg_multi_fetch": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "admm_reg_multi_set_weights": (C.c_int, [C.c_void_p, _dp]),
    "admm_reg_multi_launches": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "admm_reg_multi_chunk": (C.c_int, []),
    "admm_reg_multi_destroy": (None, [C.c_void_p]),
    "admm_op_spmm": (C.c_int, [C.POINTER(SparseDesc), C.c_int, C.c_int, _dp, _dp]),
    "admm_op_spmm_weighted": (C.c_int, [C.POINTER(SparseDesc), C.c_int32, _dp, _dp, C.c_int32, C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), _dp]),
    "admm_op_spmm_cg": (C.c_int, [C.POINTER(SparseDesc), C.c_int32, _dp, _dp, C.c_double, C.c_double, C.c_int32,
                                  C.c_int32, C.POINTER(C.c_int32), _dp, _dp, C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int32)]),
    "admm_sparse_svm_desc_default": (None, [C.POINTER(SparseSvmDesc)]),
    "admm_sparse_svm_options_default": (None, [C.POINTER(SparseSvmOptions)]),
    "admm_sparse_svm_create": (C.c_int, [C.POINTER(SparseSvmDesc), C.POINTER(C.c_void_p)]),
    "admm_sparse_svm_run": (C.c_int, [C.c_void_p, C.POINTER(SparseSvmOptions), C.POINTER(SparseSvmSummary),
                                      C.POINTER(C.c_double)]),
    "admm_sparse_svm_fetch": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "admm_sparse_svm_set_cost": (C.c_int, [C.c_void_p, _dp, _dp]),
    "admm_sparse_svm_chunk": (C.c_int, []),
    "admm_sparse_svm_destroy": (None, [C.c_void_p]),
    "admm_sparse_reg_desc_default": (None, [C.POINTER(SparseRegDesc)]),
    "admm_sparse_reg_options_default": (None, [C.POINTER(SparseRegOptions)]),
    "admm_sparse_reg_create": (C.c_int, [C.POINTER(SparseRegDesc), C.POINTER(C.c_void_p)]),
    "admm_sparse_reg_run": (C.c_int, [C.c_void_p, C.POINTER(SparseRegOptions), C.POINTER(SparseRegSummary),
                                      C.POINTER(C.c_double)]),
    "admm_sparse_reg_fetch": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "admm_sparse_reg_set_weights": (C.c_int, [C.c_void_p, _dp]),
    "admm_sparse_reg_chunk": (C.c_int, []),
    "admm_sparse_reg_destroy": (None, [C.c_void_p]),
    "admm_sparse_lasso_desc_default": (None, [C.POINTER(SparseLassoDesc)]),
    "admm_sparse_lasso_options_default": (None, [C.POINTER(SparseLassoOptions)]),
    "admm_sparse_lasso_create": (C.c_int, [C.POINTER(SparseLassoDesc), C.POINTER(C.c_void_p)]),
    "admm_sparse_lasso_run": (C.c_int, [C.c_void_p, C.POINTER(SparseLassoOptions), C.POINTER(SparseLassoSummary),
                                        C.POINTER(C.c_double)]),
    "admm_sparse_lasso_fetch": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "admm_sparse_lasso_set_weights": (C.c_int, [C.c_void_p, _dp]),
    "admm_sparse_lasso_set_groups": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), _dp, _dp]),
    "admm_sparse_lasso_set_observations": (C.c_int, [C.c_void_p, _dp, C.c_int32, C.POINTER(C.c_int32),
                                                     C.POINTER(C.c_int32)]),
    "admm_sparse_lasso_heldout": (C.c_int, [C.c_void_p, _dp, _dp]),
    "admm_sparse_lasso_chunk": (C.c_int, []),
    "admm_sparse_lasso_destroy": (None, [C.c_void_p]),
    "admm_lasso_multi_desc_default": (None, [C.POINTER(LassoMultiDesc)]),
    "admm_lasso_multi_options_default": (None, [C.POINTER(LassoMultiOptions)]),
    "admm_lasso_multi_create": (C.c_int, [C.POINTER(LassoMultiDesc), C.POINTER(C.c_void_p)]),
    "admm_lasso_multi_run": (C.c_int, [C.c_void_p, C.POINTER(LassoMultiOptions), C.POINTER(LassoMultiSummary),
                                       C.POINTER(C.c_double)]),
    "admm_lasso_multi_fetch": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "admm_lasso_multi_set_weights": (C.c_int, [C.c_void_p, _dp]),
    "admm_lasso_multi_set_groups": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), _dp, _dp]),
    "admm_group_l1class_set_groups": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), _dp, _dp]),
    "admm_sparse_l1class_set_groups": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), _dp, _dp]),
    "admm_lasso_multi_chunk": (C.c_int, []),
    "admm_lasso_multi_product_time": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                                C.POINTER(C.c_int64)]),
    "admm_lasso_multi_destroy": (None, [C.c_void_p]),
    "admm_covsel_multi_desc_default": (None, [C.POINTER(CovselMultiDesc)]),
    "admm_covsel_multi_options_default": (None, [C.POINTER(CovselMultiOptions)]),
    "admm_covsel_multi_create": (C.c_int, [C.POINTER(CovselMultiDesc), C.POINTER(C.c_void_p)]),
    "admm_covsel_multi_run": (C.c_int, [C.c_void_p, C.POINTER(CovselMultiOptions), C.POINTER(CovselMultiSummary),
                                        C.POINTER(C.c_double)]),
    "admm_covsel_multi_fetch": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "admm_covsel_multi_destroy": (None, [C.c_void_p]),
    "admm_l1class_desc_default": (None, [C.POINTER(L1ClassDesc)]),
    "admm_l1class_options_default": (None, [C.POINTER(L1ClassOptions)]),
    "admm_l1class_create": (C.c_int, [C.POINTER(L1ClassDesc), C.POINTER(C.c_void_p)]),
    "admm_l1class_run": (C.c_int, [C.c_void_p, C.POINTER(L1ClassOptions), C.POINTER(L1ClassSummary),
                                   C.POINTER(C.c_double)]),
    "admm_l1class_fetch": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "admm_l1class_set_cost": (C.c_int, [C.c_void_p, _dp, _dp]),
    "admm_l1class_set_l1weights": (C.c_int, [C.c_void_p, _dp]),
    "admm_l1class_chunk": (C.c_int, []),
    "admm_l1class_launches": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "admm_l1class_pass_time": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double),
                                         C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "admm_l1class_destroy": (None, [C.c_void_p]),
    "admm_sparse_l1class_desc_default": (None, [C.POINTER(SparseL1ClassDesc)]),
    "admm_sparse_l1class_options_default": (None, [C.POINTER(SparseL1ClassOptions)]),
    "admm_sparse_l1class_create": (C.c_int, [C.POINTER(SparseL1ClassDesc), C.POINTER(C.c_void_p)]),
    "admm_sparse_l1class_run": (C.c_int, [C.c_void_p, C.POINTER(SparseL1ClassOptions), C.POINTER(SparseL1ClassSummary),
                                          C.POINTER(C.c_double)]),
    "admm_sparse_l1class_fetch": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "admm_sparse_l1class_set_cost": (C.c_int, [C.c_void_p, _dp, _dp]),
    "admm_sparse_l1class_set_l1weights": (C.c_int, [C.c_void_p, _dp]),
    "admm_sparse_l1class_set_folds": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "admm_sparse_l1class_heldout": (C.c_int, [C.c_void_p, _dp, _dp, _dp]),
    "admm_sparse_l1class_set_multinomial": (C.c_int, [C.c_void_p, C.c_int32]),
    "admm_op_softmax_prox": (C.c_int, [_dp, C.POINTER(C.c_int32), _dp, C.c_int64, C.c_int32, _dp, C.POINTER(C.c_int32)]),
    "admm_sparse_l1class_chunk": (C.c_int, []),
    "admm_sparse_l1class_kernel_time": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double),
                                                  C.POINTER(C.c_double)]),
    "admm_sparse_l1class_destroy": (None, [C.c_void_p]),
    "admm_op_symm_packed": (C.c_int, [_dp, C.c_int64, C.c_int64, _dp, C.c_int32, C.POINTER(C.c_int32), _dp]),
    "admm_op_group_soft_threshold_multi": (C.c_int, [_dp, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.c_int32, _dp, _dp,
                                                     C.POINTER(C.c_int32), _dp]),
    "admm_group_multi_plan": (C.c_int, [C.c_int64, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_int64), C.c_int32,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def load():
    """Load libadmm_hip.so (once).  Raises AdmmError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AdmmError(E_DEVICE, f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                                  f"g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    if os.environ.get("ADMM_HIP_NO_TORCH") != "1":
        # torch ships its own HIP runtime (torch/lib/libamdhip64.so).  Whichever runtime is loaded first owns
        # the GPU: if ours (/opt/rocm) came first, torch would later report "No HIP GPUs are available" and
        # RCCL sharing / device-tensor prox callbacks could not work.  Importing torch first makes
        # libadmm_hip.so bind to the runtime already in the process (same soname).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.admm_abi_version() != ABI_VERSION:
        raise AdmmError(E_INVALID, "libadmm_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc):
    if rc != OK:
        msg = load().admm_last_error()
        raise AdmmError(rc, msg.decode("utf-8", "replace") if msg else "unknown error")


def device_count():
    n = C.c_int(0)
    rc = load().admm_device_count(C.byref(n))
    return n.value if rc == OK else 0


def require_device():
    if device_count() <= 0:
        raise AdmmError(E_DEVICE, "no HIP device visible: the ADMM engine has no CPU fallback")


def as_dp(a):
    return a.ctypes.data_as(_dp)
