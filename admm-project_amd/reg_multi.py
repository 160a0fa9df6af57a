"""Python owner of one ``admm_reg_multi`` handle (include/admm_engine.h): K quantile / LAD / Huber fits
over one design matrix D, every fit a plain-ADMM run that stops on pnorm < perr (``nodualerror = 1``)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import _MultiOwner, _f64, _weights

KINDS = {"lad": L.REGM_KIND_LAD, "huber": L.REGM_KIND_HUBER, "huberfit": L.REGM_KIND_HUBER}


class RegMulti(_MultiOwner):
    """``RegMulti(D, S, kinds, a, b, epsilon, delta)``: ``S`` is m x 1 (one response shared by all fits) or m x K (one
    column per fit); ``kinds`` holds K entries 0 | 1 (or 'lad' | 'huber'); ``a``, ``b``, ``epsilon``, ``delta`` K values
    each, or None for the defaults 1, 1, 0, 1."""

    _abi, _unit = "admm_reg_multi", "fit"

    def __init__(self, D, S, kinds, a=None, b=None, epsilon=None, delta=None, *, device=0):
        self._h = None
        self._lib = L.load()
        L.require_device()
        D = _f64(D)
        S = np.asarray(S, dtype=np.float64)
        S = _f64(S.reshape(-1, 1) if S.ndim == 1 else S)
        if S.ndim != 2 or S.shape[0] != D.shape[0]:
            raise ValueError("The number of rows in argument D do not match size of S!")
        self.m, self.n = (int(v) for v in D.shape)
        kind = np.ascontiguousarray([KINDS.get(v, v) if isinstance(v, str) else int(v) for v in kinds], dtype=np.int32)
        self.K = int(kind.size)
        d = L.RegMultiDesc()
        self._lib.admm_reg_multi_desc_default(C.byref(d))
        d.K, d.m, d.n = self.K, self.m, self.n
        d.D, d.ldD, d.S, d.ns = L.as_dp(D), self.m, L.as_dp(S), int(S.shape[1])
        d.kind = kind.ctypes.data_as(C.POINTER(C.c_int32))
        d.mem, d.device = L.MEM_HOST, int(device)
        keep = []
        for name, v in (("a", a), ("b", b), ("epsilon", epsilon), ("delta", delta)):
            if v is not None:
                arr = _weights(v, self.K, "fits", name)
                keep.append(arr)
                setattr(d, name, L.as_dp(arr))
        h = C.c_void_p()
        L.check(self._lib.admm_reg_multi_create(C.byref(d), C.byref(h)))
        self._h = h
        self.objevals = False

    @staticmethod
    def chunk():
        """fits one pass over D serves"""
        return int(L.load().admm_reg_multi_chunk())

    def set_weights(self, weights=None):
        """m observation weights >= 0 shared by all fits (admm_reg_multi_set_weights); None restores 1"""
        w = _weights(weights, self.m, "observations")
        L.check(self._lib.admm_reg_multi_set_weights(self._h, None if w is None else L.as_dp(w)))

    def run(self, *, rho=1.0, maxiters=1000, abstol=1e-5, reltol=1e-3, relax=1.0, fast=L.FAST_OFF, convtest=0,
            domaxiters=0, objevals=0, check_every=0, x0=None, z0=None, u0=None):
        o = L.RegMultiOptions()
        self._lib.admm_reg_multi_options_default(C.byref(o))
        o.maxiters, o.rho, o.abstol, o.reltol = int(maxiters), float(rho), float(abstol), float(reltol)
        o.relax, o.fast, o.convtest = float(relax), int(fast), int(bool(convtest))
        o.domaxiters, o.objevals, o.check_every = int(bool(domaxiters)), int(bool(objevals)), int(check_every)
        keep = self._start_vectors(o, x0=x0, z0=z0, u0=u0)  # noqa: F841 (alive until the run returns)
        summ = (L.RegMultiSummary * self.K)()
        rt = C.c_double(0)
        L.check(self._lib.admm_reg_multi_run(self._h, C.byref(o), summ, C.byref(rt)))
        self.objevals = bool(objevals)
        return self._summary(summ, rt)

    def launches(self):
        """kernel launches of the last run's iterations: dict(iterations, xsolve, passes, finalize, explicit_map)"""
        c = (C.c_int64 * 5)()
        L.check(self._lib.admm_reg_multi_launches(self._h, c))
        return dict(iterations=int(c[0]), xsolve=int(c[1]), passes=int(c[2]), finalize=int(c[3]),
                    explicit_map=bool(c[4]))
