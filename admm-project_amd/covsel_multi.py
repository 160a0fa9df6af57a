"""Python owner of one ``admm_covsel_multi`` handle (include/admm_engine.h): K covariance-selection fits
over one S -- a regularisation path or a cross-validation grid -- every fit a plain-ADMM run of the n x n iterates in one
workgroup of its own, the whole iteration in one kernel (csrc/covsel_multi.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import _MultiOwner, _f64, _weights


class CovselMulti(_MultiOwner):
    """``CovselMulti(lams, D=, S=)``: ``D`` holds m samples of n variables (S = cov(D) is built on the device), or ``S``
    is the n x n symmetric matrix itself; exactly one of the two.  ``lams`` holds the K values lambda_k > 0.  n <= 96."""

    _abi, _unit = "admm_covsel_multi", "fit"
    _types = (L.CovselMultiDesc, L.CovselMultiOptions, L.CovselMultiSummary)
    _rows = dict(z0="nn", u0="nn", rhos="_one")  # z and u are n x n, flattened column by column; rhos is 1 x K
    _one = 1
    _fields = dict(xopt=(L.CM_F_XOPT, "nn"), zopt=(L.CM_F_ZOPT, "nn"), uopt=(L.CM_F_UOPT, "nn"),
                   pnorm=(L.CM_F_PNORM, "hist"), perr=(L.CM_F_PERR, "hist"), dnorm=(L.CM_F_DNORM, "dual"),
                   derr=(L.CM_F_DERR, "dual"), objevals=(L.CM_F_OBJEVALS, "objevals"))
    _chunk_result = False  # (nothing is chunked: a fit is a workgroup)

    def __init__(self, lams, D=None, S=None, *, device=0):
        d = self._desc()
        if (D is None) == (S is None):
            raise ValueError("CovselMulti takes either the samples D or the matrix S")
        lam = np.ascontiguousarray(np.asarray(lams, dtype=np.float64).reshape(-1))
        self.K = int(lam.size)
        if D is not None:
            D = _f64(D)
            if D.ndim != 2:
                raise ValueError("Argument D is not a matrix!")
            self.m, self.n = (int(v) for v in D.shape)
            d.D, d.ldD = L.as_dp(D), self.m
        else:
            S = _f64(S)
            if S.ndim != 2 or S.shape[0] != S.shape[1]:
                raise ValueError("S is not a square matrix")
            self.m, self.n = 0, int(S.shape[0])
            d.S = L.as_dp(S)
        self.nn = self.n * self.n
        d.K, d.m, d.n, d.lam, d.device = self.K, self.m, self.n, L.as_dp(lam), int(device)
        self._create(d)
        self.dual = True

    def cov(self):
        """S as the object holds it (n x n): cov(D) as built on the device, or the caller's S"""
        buf = np.empty((self.n, self.n), dtype=np.float64, order="F")
        w = C.c_size_t(0)
        L.check(self._lib.admm_covsel_multi_fetch(self._h, L.CM_F_COV, L.as_dp(buf), buf.size, C.byref(w)))
        assert w.value == buf.size, (w.value, buf.size)
        return buf

    def run(self, *, rhos=None, nodualerror=0, z0=None, u0=None, **loop):
        """``rhos``: K values rho_k > 0 (None: ``rho`` for every fit); ``z0`` / ``u0``: n x n x K or n*n x K (None:
        zeros).  ``loop``: rho, maxiters, abstol, reltol, relax, fast, convtest, domaxiters, objevals, check_every"""
        r = _weights(rhos, self.K, "fits", "rhos")
        starts = {}
        for name, v in (("z0", z0), ("u0", u0)):
            if v is None:
                continue
            v = np.asarray(v, dtype=np.float64)
            if v.shape == (self.n, self.n, self.K):
                v = v.reshape((self.nn, self.K), order="F")
            elif v.shape != (self.nn, self.K):
                raise ValueError(f"{name} is not an {self.n} x {self.n} x {self.K} array (one n x n start per fit)")
            starts[name] = v
        if r is not None:
            starts["rhos"] = r.reshape(1, self.K)  # (a K-vector option travels as the start matrices do)
        return self._run(loop, starts, nodualerror=nodualerror)

    @staticmethod
    def _summary(summ, rt, cg=False):
        out = _MultiOwner._summary(summ, rt, cg)
        out["jacobi_sweeps"] = np.array([s.jacobi_sweeps for s in summ], dtype=np.int64)
        return out

    def results(self, summ):
        """_MultiOwner.results with xopt / zopt / uopt as n x n x K, plus jacobi_sweeps (K)"""
        kept = dict(hist=int(summ["steps"].max()))
        if self.objevals:
            kept["objevals"] = kept["hist"]
        if self.dual:
            kept["dual"] = kept["hist"]
        res = {}
        for key in ("xopt", "zopt", "uopt"):
            res[key] = self.fetch(self._fields[key][0], self.nn).reshape((self.n, self.n, self.K), order="F")
        res["steps"] = summ["steps"]
        res.update({key: self.fetch(field, kept[rows]) for key, (field, rows) in self._fields.items() if rows in kept})
        res.update(objopt=summ["objopt"], runtime=summ["runtime"], jacobi_sweeps=summ["jacobi_sweeps"])
        return res
