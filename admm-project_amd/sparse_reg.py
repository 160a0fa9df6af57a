"""Python owner of one ``admm_sparse_reg`` handle (include/admm_engine.h): K quantile / LAD / Huber fits
over one SPARSE design matrix, every fit a plain-ADMM run whose x-update is conjugate gradients on
D'D x = D'(s + z - u), all fits in lock-step over one sparse product."""
from __future__ import annotations

import ctypes as C

from . import _lib as L
from .engine import _MultiOwner
from .reg_multi import RegMulti


class SparseRegMulti(_MultiOwner):
    """``SparseRegMulti(D, S, kinds, a, b, epsilon, delta)``: ``D`` any ``scipy.sparse`` matrix or array (converted to
    canonical CSC); ``S`` is m x 1 (one response shared by all fits) or m x K (one column per fit); ``kinds`` holds K
    entries 0 | 1 (or 'lad' | 'huber'); ``a``, ``b``, ``epsilon``, ``delta`` K values each, or None for 1, 1, 0, 1."""

    _abi, _unit, _cg = "admm_sparse_reg", "fit", True
    _types = (L.SparseRegDesc, L.SparseRegOptions, L.SparseRegSummary)
    _fields = dict(xopt=(L.SRG_F_XOPT, "n"), zopt=(L.SRG_F_ZOPT, "m"), uopt=(L.SRG_F_UOPT, "m"),
                   pnorm=(L.SRG_F_PNORM, "hist"), perr=(L.SRG_F_PERR, "hist"), dnorm=(L.SRG_F_DNORM, "dual"),
                   derr=(L.SRG_F_DERR, "dual"), objevals=(L.SRG_F_OBJEVALS, "objevals"))
    _fit_fields, set_weights = RegMulti._fit_fields, RegMulti.set_weights

    def __init__(self, D, S, kinds, a=None, b=None, epsilon=None, delta=None, *, device=0):
        d = self._desc()
        keep = []
        sd, S = self._sparse_D(D, S, keep, "The number of rows in argument D do not match size of S!")
        d.D = C.pointer(sd)
        keep += self._fit_fields(d, S, kinds, a, b, epsilon, delta, device)
        self._create(d)
        self.dual = False

    def run(self, *, cg_tol=0.0, cg_maxit=0, nodualerror=1, z0=None, u0=None, **loop):
        """``loop``: rho, maxiters, abstol, reltol, relax, fast, convtest, domaxiters, objevals, check_every;
        cg_tol / cg_maxit <= 0: the defaults 1e-12, 200"""
        return self._run(loop, dict(z0=z0, u0=u0), cg_tol=cg_tol, cg_maxit=cg_maxit, nodualerror=nodualerror)
