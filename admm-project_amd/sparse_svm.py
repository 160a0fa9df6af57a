"""Python owner of one ``admm_sparse_svm`` handle (include/admm_engine.h): the linear SVM for K
one-vs-rest classes over one SPARSE design matrix, every class a plain-ADMM run whose x-update is conjugate gradients
on D'D x = D'(z - u), all classes in lock-step over one sparse product."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import _MultiOwner, _f64, _weights


class SparseSvmOvr(_MultiOwner):
    """``SparseSvmOvr(D, ELL, C, losses)``: ``D`` any ``scipy.sparse`` matrix or array (converted to canonical CSC),
    ``ELL`` m x K labels +-1, ``losses`` K strings ('hinge', '01', 'logistic', 'sqhinge')."""

    _abi, _unit = "admm_sparse_svm", "class"

    def __init__(self, D, ELL, C_, losses, *, device=0):
        self._h = None
        self._lib = L.load()
        L.require_device()
        keep = []
        sd = L.sparse_desc(D, keep)
        ELL = _f64(ELL.reshape(-1, 1) if np.ndim(ELL) == 1 else ELL)
        self.m, self.n, self.nnz = int(sd.rows), int(sd.cols), int(sd.nnz)
        if ELL.ndim != 2 or ELL.shape[0] != self.m:
            raise ValueError("Product ell*D is not possible; sizes incompatible!")
        self.K = int(ELL.shape[1])
        loss = np.ascontiguousarray([L.loss_code(v) for v in losses], dtype=np.int32)
        if loss.size != self.K:
            raise ValueError(f"{loss.size} losses for {self.K} classes")
        d = L.SparseSvmDesc()
        self._lib.admm_sparse_svm_desc_default(C.byref(d))
        d.K, d.D, d.ELL = self.K, C.pointer(sd), L.as_dp(ELL)
        d.loss = loss.ctypes.data_as(C.POINTER(C.c_int32))
        d.C, d.device = float(C_), int(device)
        h = C.c_void_p()
        L.check(self._lib.admm_sparse_svm_create(C.byref(d), C.byref(h)))
        self._h = h
        self.objevals = False

    @staticmethod
    def chunk():
        """classes one sparse product serves"""
        return int(L.load().admm_sparse_svm_chunk())

    def set_cost(self, weights=None, classcost=None):
        """The costs of the K classes (admm_sparse_svm_set_cost): ``weights`` = m values >= 0 shared by all classes,
        ``classcost`` = a K x 2 array, row c = (cost_pos, cost_neg) of class c.  None: the defaults (1)."""
        w = _weights(weights, self.m, "observations")
        cc = None if classcost is None else np.ascontiguousarray(np.asarray(classcost, dtype=np.float64))
        if cc is not None and cc.shape != (self.K, 2):
            raise ValueError(f"classcost is not a {self.K} x 2 array (one (pos, neg) pair per class)")
        L.check(self._lib.admm_sparse_svm_set_cost(self._h, None if w is None else L.as_dp(w),
                                                   None if cc is None else L.as_dp(cc)))

    def run(self, *, rho=1.0, maxiters=1000, abstol=1e-5, reltol=1e-3, Hnormtol=1e-6, relax=1.0, fast=L.FAST_OFF,
            convtest=0, domaxiters=0, objevals=0, check_every=0, cg_tol=0.0, cg_maxit=0, z0=None, u0=None):
        o = L.SparseSvmOptions()
        self._lib.admm_sparse_svm_options_default(C.byref(o))
        o.maxiters, o.rho, o.abstol, o.reltol, o.Hnormtol = int(maxiters), float(rho), float(abstol), float(reltol), \
            float(Hnormtol)
        o.relax, o.fast, o.convtest = float(relax), int(fast), int(bool(convtest))
        o.domaxiters, o.objevals, o.check_every = int(bool(domaxiters)), int(bool(objevals)), int(check_every)
        o.cg_tol, o.cg_maxit = float(cg_tol), int(cg_maxit)  # (<= 0: the defaults 1e-12, 200)
        keep = self._start_vectors(o, z0=z0, u0=u0)  # noqa: F841 (alive until the run returns)
        summ = (L.SparseSvmSummary * self.K)()
        rt = C.c_double(0)
        L.check(self._lib.admm_sparse_svm_run(self._h, C.byref(o), summ, C.byref(rt)))
        self.objevals = bool(objevals)
        return self._summary(summ, rt, cg=True)
