"""Python owner of one ``admm_sparse_reg`` handle (include/admm_engine.h): K quantile / LAD / Huber fits
over one SPARSE design matrix, every fit a plain-ADMM run whose x-update is conjugate gradients on
D'D x = D'(s + z - u), all fits in lock-step over one sparse product."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import _MultiOwner, _f64, _weights
from .reg_multi import KINDS


class SparseRegMulti(_MultiOwner):
    """``SparseRegMulti(D, S, kinds, a, b, epsilon, delta)``: ``D`` any ``scipy.sparse`` matrix or array (converted to
    canonical CSC); ``S`` is m x 1 (one response shared by all fits) or m x K (one column per fit); ``kinds`` holds K
    entries 0 | 1 (or 'lad' | 'huber'); ``a``, ``b``, ``epsilon``, ``delta`` K values each, or None for 1, 1, 0, 1."""

    _abi, _unit = "admm_sparse_reg", "fit"

    def __init__(self, D, S, kinds, a=None, b=None, epsilon=None, delta=None, *, device=0):
        self._h = None
        self._lib = L.load()
        L.require_device()
        keep = []
        sd = L.sparse_desc(D, keep)
        S = np.asarray(S, dtype=np.float64)
        S = _f64(S.reshape(-1, 1) if S.ndim == 1 else S)
        self.m, self.n, self.nnz = int(sd.rows), int(sd.cols), int(sd.nnz)
        if S.ndim != 2 or S.shape[0] != self.m:
            raise ValueError("The number of rows in argument D do not match size of S!")
        kind = np.ascontiguousarray([KINDS.get(v, v) if isinstance(v, str) else int(v) for v in kinds], dtype=np.int32)
        self.K = int(kind.size)
        d = L.SparseRegDesc()
        self._lib.admm_sparse_reg_desc_default(C.byref(d))
        d.K, d.D, d.S, d.ns = self.K, C.pointer(sd), L.as_dp(S), int(S.shape[1])
        d.kind = kind.ctypes.data_as(C.POINTER(C.c_int32))
        d.device = int(device)
        for name, v in (("a", a), ("b", b), ("epsilon", epsilon), ("delta", delta)):
            if v is not None:
                arr = _weights(v, self.K, "fits", name)
                keep.append(arr)
                setattr(d, name, L.as_dp(arr))
        h = C.c_void_p()
        L.check(self._lib.admm_sparse_reg_create(C.byref(d), C.byref(h)))
        self._h = h
        self.objevals = False
        self.dual = False

    @staticmethod
    def chunk():
        """fits one sparse product serves"""
        return int(L.load().admm_sparse_reg_chunk())

    def set_weights(self, weights=None):
        """m observation weights >= 0 shared by all fits (admm_sparse_reg_set_weights); None restores 1"""
        w = _weights(weights, self.m, "observations")
        L.check(self._lib.admm_sparse_reg_set_weights(self._h, None if w is None else L.as_dp(w)))

    def run(self, *, rho=1.0, maxiters=1000, abstol=1e-5, reltol=1e-3, relax=1.0, fast=L.FAST_OFF, convtest=0,
            domaxiters=0, objevals=0, check_every=0, cg_tol=0.0, cg_maxit=0, nodualerror=1, z0=None, u0=None):
        o = L.SparseRegOptions()
        self._lib.admm_sparse_reg_options_default(C.byref(o))
        o.maxiters, o.rho, o.abstol, o.reltol = int(maxiters), float(rho), float(abstol), float(reltol)
        o.relax, o.fast, o.convtest = float(relax), int(fast), int(bool(convtest))
        o.domaxiters, o.objevals, o.check_every = int(bool(domaxiters)), int(bool(objevals)), int(check_every)
        o.cg_tol, o.cg_maxit = float(cg_tol), int(cg_maxit)  # (<= 0: the defaults 1e-12, 200)
        o.nodualerror = int(bool(nodualerror))
        keep = self._start_vectors(o, z0=z0, u0=u0)  # noqa: F841 (alive until the run returns)
        summ = (L.SparseRegSummary * self.K)()
        rt = C.c_double(0)
        L.check(self._lib.admm_sparse_reg_run(self._h, C.byref(o), summ, C.byref(rt)))
        self.objevals = bool(objevals)
        self.dual = not bool(nodualerror)
        return self._summary(summ, rt, cg=True)
