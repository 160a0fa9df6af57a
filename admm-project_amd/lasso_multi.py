"""Python owner of one ``admm_lasso_multi`` handle (include/admm_engine.h): K lasso fits over one DENSE
design matrix -- a regularisation path, a cross-validation grid or several response columns -- every fit a plain-ADMM run
whose x-update applies the cached inverse of D'D + rho*I, read once per chunk of fits (csrc/symm.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import _MultiOwner, _set_multi_groups, _f64, _weights

_XSOLVE = dict(auto=L.XSOLVE_AUTO, inverse=L.XSOLVE_INVERSE, trsv=L.XSOLVE_TRSV)


def xsolve_code(xsolve):
    """options['xsolve'] of the dense multi-lasso: 'auto' | 'inverse' | 'trsv'"""
    if not (isinstance(xsolve, str) and xsolve.lower() in _XSOLVE):
        raise ValueError(f"options.xsolve = {xsolve!r}: the dense multi-lasso applies the cached factor "
                         "('auto', 'inverse' or 'trsv')")
    return _XSOLVE[xsolve.lower()]


class LassoMulti(_MultiOwner):
    """``LassoMulti(D, S, lams, ridge, nonnegative, l1weights, rho=, xsolve=)``: ``D`` a dense m x n matrix, m >= n;
    ``S`` is m x 1 (one response shared by all fits) or m x K (one column per fit); ``lams`` holds the K values
    lambda_k >= 0; ``ridge`` (mu_k >= 0) and ``nonnegative`` (0 | 1) K values each, or None for 0; ``l1weights`` n values
    w_i >= 0 shared by all fits, or None for 1.  ``rho`` is the rho of the cached factor and of every run."""

    _abi, _unit = "admm_lasso_multi", "fit"
    _types = (L.LassoMultiDesc, L.LassoMultiOptions, L.LassoMultiSummary)
    _rows = dict(x0="n", z0="n", u0="n")  # z and u live on the coefficients
    _fields = dict(xopt=(L.LM_F_XOPT, "n"), zopt=(L.LM_F_ZOPT, "n"), uopt=(L.LM_F_UOPT, "n"),
                   pnorm=(L.LM_F_PNORM, "hist"), perr=(L.LM_F_PERR, "hist"), dnorm=(L.LM_F_DNORM, "dual"),
                   derr=(L.LM_F_DERR, "dual"), objevals=(L.LM_F_OBJEVALS, "objevals"))

    def __init__(self, D, S, lams, ridge=None, nonnegative=None, l1weights=None, *, rho=1.0, xsolve="auto", device=0):
        d = self._desc()
        keep = []
        D = _f64(D)
        S = np.asarray(S, dtype=np.float64)
        S = _f64(S.reshape(-1, 1) if S.ndim == 1 else S)
        self.m, self.n = (int(v) for v in D.shape)
        if S.ndim != 2 or S.shape[0] != self.m:
            raise ValueError("The number of rows in argument D do not match size of S!")
        lam = np.ascontiguousarray(np.asarray(lams, dtype=np.float64).reshape(-1))
        self.K = int(lam.size)
        d.K, d.m, d.n, d.D, d.ldD = self.K, self.m, self.n, L.as_dp(D), self.m
        d.S, d.ns = L.as_dp(S), int(S.shape[1])
        d.lam = L.as_dp(lam)
        d.rho, d.xsolve, d.device = float(rho), xsolve_code(xsolve), int(device)
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
        self._create(d)
        self.rho = float(rho)
        self.dual = True
        self.xsolve = None  # 'inverse' | 'trsv' once a run has reported it

    set_groups = _set_multi_groups

    def set_weights(self, l1weights=None):
        """n l1 weights >= 0 shared by all fits (admm_lasso_multi_set_weights); None restores 1"""
        w = _weights(l1weights, self.n, "coefficients", "l1weights")
        L.check(self._lib.admm_lasso_multi_set_weights(self._h, None if w is None else L.as_dp(w)))

    def product_time(self, reps=20):
        """the packed product of the x-update alone, event-timed (admm_lasso_multi_product_time):
        dict(us, stored_bytes, fma).  Overwrites x: call it between runs."""
        us, nbytes, fma = C.c_double(0), C.c_int64(0), C.c_int64(0)
        L.check(self._lib.admm_lasso_multi_product_time(self._h, int(reps), C.byref(us), C.byref(nbytes), C.byref(fma)))
        return dict(us=us.value, stored_bytes=nbytes.value, fma=fma.value)

    def run(self, *, nodualerror=0, z0=None, u0=None, **loop):
        """``loop``: rho (default: the object's; any other value is refused), maxiters, abstol, reltol, relax, fast,
        convtest, domaxiters, objevals, check_every"""
        loop.setdefault("rho", self.rho)
        return self._run(loop, dict(z0=z0, u0=u0), nodualerror=nodualerror)

    def _summary(self, summ, rt, cg=False):
        self.xsolve = "inverse" if summ[0].xsolve == L.XSOLVE_INVERSE else "trsv"
        return _MultiOwner._summary(summ, rt, cg)

    def results(self, summ):
        res = super().results(summ)
        res["xsolve"] = self.xsolve
        return res
