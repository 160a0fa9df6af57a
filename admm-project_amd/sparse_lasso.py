"""Python owner of one ``admm_sparse_lasso`` handle (include/admm_engine.h): K lasso fits over one SPARSE
design matrix -- a regularisation path, a cross-validation grid or several response columns -- every fit a plain-ADMM run
whose x-update is conjugate gradients on (D'D + rho*I) x = D's + rho*(z - u), all fits in lock-step over one sparse
product."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import _MultiOwner, _set_multi_groups, _weights


def _int_ids(a, count, what, name):
    """integer ids as contiguous int32: ``count`` entries, one per ``what``; a non-integer value is a ValueError (a cast
    would truncate 1.5 to 1 without a word)"""
    v = np.asarray(a)
    if v.dtype == object or not (np.issubdtype(v.dtype, np.integer) or np.issubdtype(v.dtype, np.floating)
                                 or v.dtype == np.bool_):
        raise ValueError(f"{name} must hold integers")
    v = v.reshape(-1)
    if v.size != count:
        raise ValueError(f"{name} has {v.size} entries for {count} {what}")
    g = v.astype(np.float64)
    if not np.all(np.isfinite(g)) or np.any(g != np.floor(g)) or np.any(np.abs(g) >= 2.0 ** 31):
        raise ValueError(f"{name} must hold integers")
    return np.ascontiguousarray(g.astype(np.int32))


def observation_arrays(obsweights, fold, heldout, m, K):
    """(obsweights float64 | None, fold int32 | None, heldout int32 | None, nfolds) with the shape and dtype checks of
    ``SparseLassoMulti.set_observations``, each a ValueError that names its argument; the values are the library's to
    check, except what needs no device and no library: heldout without fold"""
    w = _weights(obsweights, m, "observations", "obsweights")
    f = None if fold is None else _int_ids(fold, m, "observations", "foldid")
    h = None if heldout is None else _int_ids(heldout, K, "fits", "heldout")
    if h is not None and f is None:
        raise ValueError("heldout needs foldid: the fold of every observation")
    nfolds = 0 if f is None else int(max(int(f.max(initial=-1)) + 1, 1))
    return w, f, h, nfolds


class SparseLassoMulti(_MultiOwner):
    """``SparseLassoMulti(D, S, lams, ridge, nonnegative, l1weights)``: ``D`` any ``scipy.sparse`` matrix or array
    (converted to canonical CSC); ``S`` is m x 1 (one response shared by all fits) or m x K (one column per fit);
    ``lams`` holds the K values lambda_k >= 0; ``ridge`` (mu_k >= 0) and ``nonnegative`` (0 | 1) K values each, or None
    for 0; ``l1weights`` n values w_i >= 0 shared by all fits, or None for 1."""

    _abi, _unit, _cg = "admm_sparse_lasso", "fit", True
    _types = (L.SparseLassoDesc, L.SparseLassoOptions, L.SparseLassoSummary)
    _rows = dict(x0="n", z0="n", u0="n")  # z and u live on the coefficients
    _fields = dict(xopt=(L.SLM_F_XOPT, "n"), zopt=(L.SLM_F_ZOPT, "n"), uopt=(L.SLM_F_UOPT, "n"),
                   pnorm=(L.SLM_F_PNORM, "hist"), perr=(L.SLM_F_PERR, "hist"), dnorm=(L.SLM_F_DNORM, "dual"),
                   derr=(L.SLM_F_DERR, "dual"), objevals=(L.SLM_F_OBJEVALS, "objevals"))

    def __init__(self, D, S, lams, ridge=None, nonnegative=None, l1weights=None, *, device=0):
        d = self._desc()
        keep = []
        sd, S = self._sparse_D(D, S, keep, "The number of rows in argument D do not match size of S!")
        lam = np.ascontiguousarray(np.asarray(lams, dtype=np.float64).reshape(-1))
        self.K = int(lam.size)
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
        self._create(d)
        self.dual = True

    set_groups = _set_multi_groups

    def set_weights(self, l1weights=None):
        """n l1 weights >= 0 shared by all fits (admm_sparse_lasso_set_weights); None restores 1"""
        w = _weights(l1weights, self.n, "coefficients", "l1weights")
        L.check(self._lib.admm_sparse_lasso_set_weights(self._h, None if w is None else L.as_dp(w)))

    def set_observations(self, obsweights=None, fold=None, heldout=None):
        """Observation weights and held-out folds for every later run (admm_sparse_lasso_set_observations; DESIGN.md
        q46): ``obsweights`` = m values >= 0 shared by all fits (None: 1), ``fold`` = m integer fold ids >= 0 (None: no
        row is held out), ``heldout`` = K integers, the fold fit k leaves out or -1 (None: -1 everywhere).  All None
        restores the unweighted object."""
        w, f, h, nfolds = observation_arrays(obsweights, fold, heldout, self.m, self.K)
        ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
        L.check(self._lib.admm_sparse_lasso_set_observations(self._h, None if w is None else L.as_dp(w), nfolds, ip(f),
                                                             ip(h)))

    def heldout(self):
        """(sse, weight) of the last run under observations, K values each: the weighted squared error of zopt on the
        rows fit k held out and their total weight (admm_sparse_lasso_heldout)"""
        sse, wt = np.empty(self.K), np.empty(self.K)
        L.check(self._lib.admm_sparse_lasso_heldout(self._h, L.as_dp(sse), L.as_dp(wt)))
        return sse, wt

    def run(self, *, cg_tol=0.0, cg_maxit=0, nodualerror=0, z0=None, u0=None, **loop):
        """``loop``: rho, maxiters, abstol, reltol, relax, fast, convtest, domaxiters, objevals, check_every;
        cg_tol / cg_maxit <= 0: the defaults 1e-12, 200"""
        return self._run(loop, dict(z0=z0, u0=u0), cg_tol=cg_tol, cg_maxit=cg_maxit, nodualerror=nodualerror)
