"""Python owner of one ``admm_l1class`` handle (include/admm_engine.h): K sparse linear classifiers over
one DENSE design matrix -- the l1 / elastic-net penalty of the lasso family on the hinge, squared-hinge or logistic loss
-- every fit a plain-ADMM run with A = [D; I] whose x-update applies the cached inverse of D'D + I and whose two passes
over D serve a chunk of fits each (csrc/l1class.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import _MultiOwner, _set_multi_groups, _set_svm_cost, _f64, _weights
from .lasso_multi import xsolve_code

_LOSSES = dict(hinge=L.LOSS_HINGE, sqhinge=L.LOSS_SQHINGE, logistic=L.LOSS_LOGISTIC)


def loss_code(name, fit=None):
    """options['lossfunction'] of the l1 classifier: 'hinge' | 'sqhinge' | 'logistic'"""
    who = "" if fit is None else f"fit {fit}: "
    if not (isinstance(name, str) and name.lower() in _LOSSES):
        raise ValueError(f"{who}lossfunction = {name!r}: the l1 classifier takes 'hinge', 'sqhinge' or 'logistic' (the "
                         "0-1 loss is not convex and has no lambda_max)")
    return _LOSSES[name.lower()]


class L1Classifier(_MultiOwner):
    """``L1Classifier(D, ELL, lams, losses, ridge, nonnegative, l1weights, C=, xsolve=)``: ``D`` a dense m x n matrix
    of any shape; ``ELL`` is m x 1 (labels +-1 shared by all fits) or m x K; ``lams`` holds the K values lambda_k >= 0;
    ``losses`` K names (or None: logistic); ``ridge`` (mu_k >= 0) and ``nonnegative`` (0 | 1) K values each, or None for
    0; ``l1weights`` n values w_j >= 0 shared by all fits, or None for 1."""

    _abi, _unit = "admm_l1class", "fit"
    _set_groups_abi = "admm_group_l1class_set_groups"  # (its own prefix: include/admm_engine.h)
    _types = (L.L1ClassDesc, L.L1ClassOptions, L.L1ClassSummary)
    _rows = dict(x0="n", z0="mn", u0="mn")  # z and u stack the m rows of D above the n coefficients
    _fields = dict(xopt=(L.L1C_F_XOPT, "n"), zopt=(L.L1C_F_ZOPT, "mn"), uopt=(L.L1C_F_UOPT, "mn"),
                   pnorm=(L.L1C_F_PNORM, "hist"), perr=(L.L1C_F_PERR, "hist"), dnorm=(L.L1C_F_DNORM, "dual"),
                   derr=(L.L1C_F_DERR, "dual"), objevals=(L.L1C_F_OBJEVALS, "objevals"))

    def __init__(self, D, ELL, lams, losses=None, ridge=None, nonnegative=None, l1weights=None, *, C=1.0, xsolve="auto",
                 device=0):
        d = self._desc()
        keep = []
        D = _f64(D)
        ELL = np.asarray(ELL, dtype=np.float64)
        ELL = _f64(ELL.reshape(-1, 1) if ELL.ndim == 1 else ELL)
        self.m, self.n = (int(v) for v in D.shape)
        self.mn = self.m + self.n
        if ELL.ndim != 2 or ELL.shape[0] != self.m:
            raise ValueError("The number of rows in argument D do not match size of ell!")
        lam = np.ascontiguousarray(np.asarray(lams, dtype=np.float64).reshape(-1))
        self.K = int(lam.size)
        d.K, d.m, d.n, d.D, d.ldD = self.K, self.m, self.n, L.as_dp(D), self.m
        d.ELL, d.nell = L.as_dp(ELL), int(ELL.shape[1])
        d.lam = L.as_dp(lam)
        d.C, d.xsolve, d.device = float(C), xsolve_code(xsolve), int(device)
        if losses is not None:
            codes = [v if isinstance(v, (int, np.integer)) else loss_code(v, k) for k, v in enumerate(losses)]
            lc = np.ascontiguousarray(codes, dtype=np.int32)
            if lc.size != self.K:
                raise ValueError(f"lossfunction has {lc.size} entries for {self.K} fits")
            keep.append(lc)
            d.loss = lc.ctypes.data_as(C_INT32_P)
        if ridge is not None:
            mu = _weights(ridge, self.K, "fits", "ridge")
            keep.append(mu)
            d.ridge = L.as_dp(mu)
        if nonnegative is not None:
            nn = np.ascontiguousarray(np.asarray(nonnegative).reshape(-1), dtype=np.int32)
            if nn.size != self.K:
                raise ValueError(f"nonnegative has {nn.size} entries for {self.K} fits")
            keep.append(nn)
            d.nonneg = nn.ctypes.data_as(C_INT32_P)
        w = _weights(l1weights, self.n, "coefficients", "l1weights")
        if w is not None:
            d.l1weights = L.as_dp(w)
        self._create(d)
        self.dual = True
        self.xsolve = None  # 'inverse' | 'trsv' once a run has reported it

    set_cost = _set_svm_cost
    set_groups = _set_multi_groups  # (lambda becomes the group strength, l1 the l1 strength)

    def set_l1weights(self, l1weights=None):
        """n l1 weights >= 0 shared by all fits (admm_l1class_set_l1weights); None restores 1"""
        w = _weights(l1weights, self.n, "coefficients", "l1weights")
        L.check(self._lib.admm_l1class_set_l1weights(self._h, None if w is None else L.as_dp(w)))

    def launches(self):
        """(kernel launches of the last run, how many of them read D)"""
        a, b = C.c_int64(0), C.c_int64(0)
        L.check(self._lib.admm_l1class_launches(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def pass_time(self, reps=20, nvec=1):
        """the two passes over D alone, one chunk, event-timed (admm_l1class_pass_time): dict(forward_us,
        transposed_us, d_bytes).  Overwrites the iterates: call it between runs."""
        f, t, nb = C.c_double(0), C.c_double(0), C.c_int64(0)
        L.check(self._lib.admm_l1class_pass_time(self._h, int(reps), int(nvec), C.byref(f), C.byref(t), C.byref(nb)))
        return dict(forward_us=f.value, transposed_us=t.value, d_bytes=nb.value)

    def run(self, *, nodualerror=0, z0=None, u0=None, **loop):
        """``loop``: rho, maxiters, abstol, reltol, relax, fast, convtest, domaxiters, objevals, check_every"""
        return self._run(loop, dict(z0=z0, u0=u0), nodualerror=nodualerror)

    def _summary(self, summ, rt, cg=False):
        self.xsolve = "inverse" if summ[0].xsolve == L.XSOLVE_INVERSE else "trsv"
        return _MultiOwner._summary(summ, rt, cg)

    def results(self, summ):
        res = super().results(summ)
        res["xsolve"] = self.xsolve
        return res


C_INT32_P = C.POINTER(C.c_int32)
