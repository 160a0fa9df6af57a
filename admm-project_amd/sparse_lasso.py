"""Python owner of one ``admm_sparse_lasso`` handle (include/admm_engine.h): K lasso fits over one SPARSE
design matrix -- a regularisation path, a cross-validation grid or several response columns -- every fit a plain-ADMM run
whose x-update is conjugate gradients on (D'D + rho*I) x = D's + rho*(z - u), all fits in lock-step over one sparse
product."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import _MultiOwner, _f64, _weights


class SparseLassoMulti(_MultiOwner):
    """``SparseLassoMulti(D, S, lams, ridge, nonnegative, l1weights)``: ``D`` any ``scipy.sparse`` matrix or array
    (converted to canonical CSC); ``S`` is m x 1 (one response shared by all fits) or m x K (one column per fit);
    ``lams`` holds the K values lambda_k >= 0; ``ridge`` (mu_k >= 0) and ``nonnegative`` (0 | 1) K values each, or None
    for 0; ``l1weights`` n values w_i >= 0 shared by all fits, or None for 1."""

    _abi, _unit = "admm_sparse_lasso", "fit"

    def __init__(self, D, S, lams, ridge=None, nonnegative=None, l1weights=None, *, device=0):
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
        lam = np.ascontiguousarray(np.asarray(lams, dtype=np.float64).reshape(-1))
        self.K = int(lam.size)
        d = L.SparseLassoDesc()
        self._lib.admm_sparse_lasso_desc_default(C.byref(d))
        d.K, d.D, d.S, d.ns = self.K, C.pointer(sd), L.as_dp(S), int(S.shape[1])
        d.lam = L.as_dp(lam)
        d.device = int(device)
        if ridge is not None:
            mu = _weights(ridge, self.K, "fits", "ridge")
            keep.append(mu)
            d.ridge = L.as_dp(mu)
        if nonnegative is not None:
            nn = np.ascontiguousarray(np.asarray(nonnegative).reshape(-1), dtype=np.int32)
            if nn.size != self.K:
                raise ValueError(f"nonnegative has {nn.size} entries for {self.K} fits")
            keep.append(nn)
            d.nonneg = nn.ctypes.data_as(C.POINTER(C.c_int32))
        w = _weights(l1weights, self.n, "coefficients", "l1weights")
        if w is not None:
            d.weights = L.as_dp(w)
        h = C.c_void_p()
        L.check(self._lib.admm_sparse_lasso_create(C.byref(d), C.byref(h)))
        self._h = h
        self.objevals = False
        self.dual = True

    @staticmethod
    def chunk():
        """fits one sparse product serves"""
        return int(L.load().admm_sparse_lasso_chunk())

    def set_weights(self, l1weights=None):
        """n l1 weights >= 0 shared by all fits (admm_sparse_lasso_set_weights); None restores 1"""
        w = _weights(l1weights, self.n, "coefficients", "l1weights")
        L.check(self._lib.admm_sparse_lasso_set_weights(self._h, None if w is None else L.as_dp(w)))

    def run(self, *, rho=1.0, maxiters=1000, abstol=1e-5, reltol=1e-3, relax=1.0, fast=L.FAST_OFF, convtest=0,
            domaxiters=0, objevals=0, check_every=0, cg_tol=0.0, cg_maxit=0, nodualerror=0, z0=None, u0=None):
        o = L.SparseLassoOptions()
        self._lib.admm_sparse_lasso_options_default(C.byref(o))
        o.maxiters, o.rho, o.abstol, o.reltol = int(maxiters), float(rho), float(abstol), float(reltol)
        o.relax, o.fast, o.convtest = float(relax), int(fast), int(bool(convtest))
        o.domaxiters, o.objevals, o.check_every = int(bool(domaxiters)), int(bool(objevals)), int(check_every)
        o.cg_tol, o.cg_maxit = float(cg_tol), int(cg_maxit)  # (<= 0: the defaults 1e-12, 200)
        o.nodualerror = int(bool(nodualerror))
        keep = []  # (alive until the run returns)
        for name, v in (("z0", z0), ("u0", u0)):  # z and u live on the coefficients: n x K
            if v is None:
                continue
            v = _f64(v)
            if v.shape != (self.n, self.K):
                raise ValueError(f"{name} is not a {self.n} x {self.K} matrix (one column per {self._unit})")
            keep.append(v)
            setattr(o, name, L.as_dp(v))
        summ = (L.SparseLassoSummary * self.K)()
        rt = C.c_double(0)
        L.check(self._lib.admm_sparse_lasso_run(self._h, C.byref(o), summ, C.byref(rt)))
        self.objevals = bool(objevals)
        self.dual = not bool(nodualerror)
        return self._summary(summ, rt, cg=True)
