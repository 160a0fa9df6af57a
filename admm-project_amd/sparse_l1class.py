"""Python owner of one ``admm_sparse_l1class`` handle (include/admm_engine.h): K sparse linear classifiers
over one SPARSE design matrix -- the l1 / elastic-net penalty of the lasso family on the hinge, squared-hinge or logistic
loss -- every fit a plain-ADMM run with A = [D; I] whose x-update is conjugate gradients on (D'D + I) x = D'(z1 - u1) +
(z2 - u2), all fits in lock-step over one sparse product (csrc/sparse_l1class.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import _MultiOwner, _set_multi_groups, _set_svm_cost, _weights
from .l1class import loss_code

_XSOLVE = dict(auto=L.XSOLVE_AUTO, cg=L.XSOLVE_CG)


class SparseL1Classifier(_MultiOwner):
    """``SparseL1Classifier(D, ELL, lams, losses, ridge, nonnegative, l1weights, C=, xsolve=)``: ``D`` any
    ``scipy.sparse`` matrix or array (converted to canonical CSC); ``ELL`` is m x 1 (labels +-1 shared by all fits) or
    m x K; ``lams`` holds the K values lambda_k >= 0; ``losses`` K names (or None: logistic); ``ridge`` (mu_k >= 0) and
    ``nonnegative`` (0 | 1) K values each, or None for 0; ``l1weights`` n values w_j >= 0 shared by all fits, or None
    for 1; ``xsolve`` 'auto' or 'cg'."""

    _abi, _unit, _cg = "admm_sparse_l1class", "fit", True
    _types = (L.SparseL1ClassDesc, L.SparseL1ClassOptions, L.SparseL1ClassSummary)
    _rows = dict(x0="n", z0="mn", u0="mn")  # z and u stack the m rows of D above the n coefficients
    _fields = dict(xopt=(L.L1C_F_XOPT, "n"), zopt=(L.L1C_F_ZOPT, "mn"), uopt=(L.L1C_F_UOPT, "mn"),
                   pnorm=(L.L1C_F_PNORM, "hist"), perr=(L.L1C_F_PERR, "hist"), dnorm=(L.L1C_F_DNORM, "dual"),
                   derr=(L.L1C_F_DERR, "dual"), objevals=(L.L1C_F_OBJEVALS, "objevals"))

    def __init__(self, D, ELL, lams, losses=None, ridge=None, nonnegative=None, l1weights=None, *, C=1.0, xsolve="auto",
                 device=0):
        d = self._desc()
        keep = []
        sd, ELL = self._sparse_D(D, ELL, keep, "The number of rows in argument D do not match size of ell!")
        self.mn = self.m + self.n
        lam = np.ascontiguousarray(np.asarray(lams, dtype=np.float64).reshape(-1))
        self.K = int(lam.size)
        if not (isinstance(xsolve, str) and xsolve.lower() in _XSOLVE):
            raise ValueError(f"xsolve = {xsolve!r}: the sparse l1 classifier runs the matrix-free x-update ('auto' or "
                             "'cg')")
        d.K, d.D, d.ELL, d.nell = self.K, C_pointer(sd), L.as_dp(ELL), int(ELL.shape[1])
        d.lam = L.as_dp(lam)
        d.C, d.xsolve, d.device = float(C), _XSOLVE[xsolve.lower()], int(device)
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

    set_cost = _set_svm_cost
    set_groups = _set_multi_groups  # (lambda becomes the group strength, l1 the l1 strength)

    def set_l1weights(self, l1weights=None):
        """n l1 weights >= 0 shared by all fits (admm_sparse_l1class_set_l1weights); None restores 1"""
        w = _weights(l1weights, self.n, "coefficients", "l1weights")
        L.check(self._lib.admm_sparse_l1class_set_l1weights(self._h, None if w is None else L.as_dp(w)))

    def set_folds(self, fold=None, heldout=None):
        """Held-out folds for every later run (admm_sparse_l1class_set_folds): ``fold`` = m integer fold
        ids >= 0 (None: no row is held out), ``heldout`` = K integers, the fold fit k leaves out or -1 (None: -1
        everywhere); a fold that no row belongs to is allowed.  A held-out row has cost 0 in its fit.  Both None restore the
        object without folds."""
        from .sparse_lasso import observation_arrays
        _, f, h, nfolds = observation_arrays(None, fold, heldout, self.m, self.K)
        if h is not None:  # (a fold without rows is a fold: its fit holds nothing out and its sums are 0)
            nfolds = max(nfolds, int(h.max(initial=-1)) + 1)
        ip = lambda a: None if a is None else a.ctypes.data_as(C_INT32_P)
        L.check(self._lib.admm_sparse_l1class_set_folds(self._h, nfolds, ip(f), ip(h)))

    def set_multinomial(self, classes=0):
        """The multinomial (softmax) loss for every later run (admm_sparse_l1class_set_multinomial):
        ``classes`` = Cn in 2 .. 10 turns the K fits into models of Cn neighbouring slots each, floor(10 / Cn) models
        per chunk of ten, the slots behind a chunk's last model idle (``softmax.slot_map``); column k of ELL is +1 on
        the rows whose class is slot k's.  A model is one ADMM problem with one stop decision, reported by each of its
        fits.  0 restores the per-fit object.  It does not combine with folds or groups."""
        L.check(self._lib.admm_sparse_l1class_set_multinomial(self._h, int(classes)))

    def heldout(self):
        """(loss, errors, weight) of the last run under folds, K values each, over the rows fit k held out, at D*z2 (z2:
        the coefficient block of zopt) with c_i = weights_i * class cost: sum c_i*phi(ell_i*t_i) without the factor C,
        sum c_i*[ell_i*t_i <= 0] and sum c_i (admm_sparse_l1class_heldout)"""
        loss, err, wt = np.empty(self.K), np.empty(self.K), np.empty(self.K)
        L.check(self._lib.admm_sparse_l1class_heldout(self._h, L.as_dp(loss), L.as_dp(err), L.as_dp(wt)))
        return loss, err, wt

    def kernel_time(self, reps=20, dual=1):
        """the row kernel (the form the object would run: with folds set, the one that reads them) and the element
        kernel alone, event-timed (admm_sparse_l1class_kernel_time): dict(row_us, elem_us).  Overwrites the iterates:
        call it between runs."""
        r, e = C.c_double(0), C.c_double(0)
        L.check(self._lib.admm_sparse_l1class_kernel_time(self._h, int(reps), int(dual), C.byref(r), C.byref(e)))
        return dict(row_us=r.value, elem_us=e.value)

    def run(self, *, cg_tol=0.0, cg_maxit=0, nodualerror=0, z0=None, u0=None, **loop):
        """``loop``: rho, maxiters, abstol, reltol, relax, fast, convtest, domaxiters, objevals, check_every;
        cg_tol / cg_maxit <= 0: the defaults 1e-12, 200"""
        return self._run(loop, dict(z0=z0, u0=u0), cg_tol=cg_tol, cg_maxit=cg_maxit, nodualerror=nodualerror)


C_INT32_P = C.POINTER(C.c_int32)
C_pointer = C.pointer
