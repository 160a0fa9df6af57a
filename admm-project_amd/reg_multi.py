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
    _types = (L.RegMultiDesc, L.RegMultiOptions, L.RegMultiSummary)
    _fields = dict(xopt=(L.REGM_F_XOPT, "n"), zopt=(L.REGM_F_ZOPT, "m"), uopt=(L.REGM_F_UOPT, "m"),
                   pnorm=(L.REGM_F_PNORM, "hist"), perr=(L.REGM_F_PERR, "hist"), objevals=(L.REGM_F_OBJEVALS, "objevals"))

    def __init__(self, D, S, kinds, a=None, b=None, epsilon=None, delta=None, *, device=0):
        d = self._desc()
        D = _f64(D)
        S = np.asarray(S, dtype=np.float64)
        S = _f64(S.reshape(-1, 1) if S.ndim == 1 else S)
        if S.ndim != 2 or S.shape[0] != D.shape[0]:
            raise ValueError("The number of rows in argument D do not match size of S!")
        self.m, self.n = (int(v) for v in D.shape)
        d.m, d.n, d.D, d.ldD, d.mem = self.m, self.n, L.as_dp(D), self.m, L.MEM_HOST
        keep = self._fit_fields(d, S, kinds, a, b, epsilon, delta, device)  # noqa: F841 (alive until create returns)
        self._create(d)

    def _fit_fields(self, d, S, kinds, a, b, epsilon, delta, device):
        """d.K, S, ns, kind, a, b, epsilon, delta and device of either regression desc; sets K and returns what must
        outlive create"""
        kind = np.ascontiguousarray([KINDS.get(v, v) if isinstance(v, str) else int(v) for v in kinds], dtype=np.int32)
        self.K = int(kind.size)
        d.K, d.S, d.ns, d.device = self.K, L.as_dp(S), int(S.shape[1]), int(device)
        d.kind = kind.ctypes.data_as(C.POINTER(C.c_int32))
        keep = [kind]
        for name, v in (("a", a), ("b", b), ("epsilon", epsilon), ("delta", delta)):
            if v is not None:
                keep.append(_weights(v, self.K, "fits", name))
                setattr(d, name, L.as_dp(keep[-1]))
        return keep

    def set_weights(self, weights=None):
        """m observation weights >= 0 shared by all fits (<abi>_set_weights); None restores 1"""
        w = _weights(weights, self.m, "observations")
        L.check(getattr(self._lib, self._abi + "_set_weights")(self._h, None if w is None else L.as_dp(w)))

    def run(self, *, x0=None, z0=None, u0=None, **loop):
        """``loop``: rho, maxiters, abstol, reltol, relax, fast, convtest, domaxiters, objevals, check_every"""
        return self._run(loop, dict(x0=x0, z0=z0, u0=u0))

    def launches(self):
        """kernel launches of the last run's iterations: dict(iterations, xsolve, passes, finalize, explicit_map)"""
        c = (C.c_int64 * 5)()
        L.check(self._lib.admm_reg_multi_launches(self._h, c))
        return dict(iterations=int(c[0]), xsolve=int(c[1]), passes=int(c[2]), finalize=int(c[3]),
                    explicit_map=bool(c[4]))
