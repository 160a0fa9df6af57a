"""Shared by the sparse-design-matrix tests: the test matrices and hand-made CSC containers."""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from admm_project_amd.binding import Sparse


def problem(ap, rows, cols, density, seed=0):
    """synth.sparse_lasso_problem's pattern with row 3 made dense, row 5 and column 7 emptied (where they exist), the
    columns renormalised, and s / lam re-derived: dict(D csc_matrix, A dense, s, lam, testx)"""
    p = ap.synth.sparse_lasso_problem(seed, rows, cols, density)
    A = p["D"].toarray()
    rng = np.random.default_rng(seed + 101)
    if rows > 3:
        A[3, :] = rng.standard_normal(cols)
    if rows > 5:
        A[5, :] = 0.0
    if cols > 7:
        A[:, 7] = 0.0
    nrm = np.sqrt(np.sum(A * A, axis=0))
    A = A / np.where(nrm > 0.0, nrm, 1.0)
    s = A @ p["testx"] + np.sqrt(0.001) * rng.standard_normal(rows)
    lam = 0.1 * float(np.max(np.abs(A.T @ s)))
    return dict(D=sp.csc_matrix(A), A=np.asfortranarray(A), s=s, lam=lam, testx=p["testx"])


class Csc(Sparse):
    """hand-made CSC arrays (possibly malformed) where binding.Sparse builds well-formed ones from a dense array"""

    def __init__(self, shape, data, ir, jc):  # (deliberately not Sparse.__init__)
        self.shape = tuple(shape)
        self.data = np.ascontiguousarray(data, dtype=np.float64)
        self.ir = np.ascontiguousarray(ir, dtype=np.uint64)
        self.jc = np.ascontiguousarray(jc, dtype=np.uint64)


def desc_of(L, csc, nnz=None, mem=None, pointers=None):
    """admm_sparse_desc over a Csc's host arrays, or over the three device ``pointers`` (val, ir, jc)"""
    d = L.SparseDesc()
    d.struct_size = C.sizeof(L.SparseDesc)
    d.mem = L.MEM_HOST if mem is None else mem
    d.rows, d.cols = csc.shape
    d.nnz = int(csc.data.size if nnz is None else nnz)
    if pointers is None:
        d.val = csc.data.ctypes.data_as(C.POINTER(C.c_double))
        d.ir = csc.ir.ctypes.data_as(C.POINTER(C.c_uint64))
        d.jc = csc.jc.ctypes.data_as(C.POINTER(C.c_uint64))
    else:
        d.val = C.cast(pointers[0], C.POINTER(C.c_double))
        d.ir = C.cast(pointers[1], C.POINTER(C.c_uint64))
        d.jc = C.cast(pointers[2], C.POINTER(C.c_uint64))
    return d


def csc_of(M):
    """a scipy.sparse matrix in canonical CSC as a Csc"""
    M = sp.csc_matrix(M, dtype=np.float64)
    M.sum_duplicates()
    M.sort_indices()
    return Csc(M.shape, M.data, M.indices, M.indptr)
