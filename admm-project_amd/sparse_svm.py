"""Python owner of one ``admm_sparse_svm`` handle (include/admm_engine.h): the linear SVM for K
one-vs-rest classes over one SPARSE design matrix, every class a plain-ADMM run whose x-update is conjugate gradients
on D'D x = D'(z - u), all classes in lock-step over one sparse product."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import _OVR_FIELDS, _MultiOwner, _set_svm_cost


class SparseSvmOvr(_MultiOwner):
    """``SparseSvmOvr(D, ELL, C, losses)``: ``D`` any ``scipy.sparse`` matrix or array (converted to canonical CSC),
    ``ELL`` m x K labels +-1, ``losses`` K strings ('hinge', '01', 'logistic', 'sqhinge')."""

    _abi, _unit, _cg = "admm_sparse_svm", "class", True
    _types = (L.SparseSvmDesc, L.SparseSvmOptions, L.SparseSvmSummary)
    _fields, _chunk_result = _OVR_FIELDS, False
    set_cost = _set_svm_cost

    def __init__(self, D, ELL, C_, losses, *, device=0):
        d = self._desc()
        keep = []
        sd, ELL = self._sparse_D(D, ELL, keep, "Product ell*D is not possible; sizes incompatible!")
        self.K = int(ELL.shape[1])
        loss = np.ascontiguousarray([L.loss_code(v) for v in losses], dtype=np.int32)
        if loss.size != self.K:
            raise ValueError(f"{loss.size} losses for {self.K} classes")
        d.K, d.D, d.ELL = self.K, C.pointer(sd), L.as_dp(ELL)
        d.loss = loss.ctypes.data_as(C.POINTER(C.c_int32))
        d.C, d.device = float(C_), int(device)
        self._create(d)

    def run(self, *, Hnormtol=1e-6, cg_tol=0.0, cg_maxit=0, z0=None, u0=None, **loop):
        """``loop``: rho, maxiters, abstol, reltol, relax, fast, convtest, domaxiters, objevals, check_every;
        cg_tol / cg_maxit <= 0: the defaults 1e-12, 200"""
        return self._run(loop, dict(z0=z0, u0=u0), Hnormtol=Hnormtol, cg_tol=cg_tol, cg_maxit=cg_maxit)
