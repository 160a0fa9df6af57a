"""The multinomial (softmax) loss on the sparse l1 classifier: ``multinomial``, ``multinomial_path``,
``multinomial_lambda_max`` and ``multinomial_proba``.  One model of Cn classes is ONE ADMM problem over x (n x Cn),

    minimise C*sum_i c_i*(logsumexp((D*x)_i,:) - (D*x)_i,y_i) + sum_c [lambda*sum_j w_j*|x_jc| + ridge/2*||x_c||^2]

(x >= 0 where nonnegative; c_i = weights_i * classweight[y_i]): glmnet's family = "multinomial" with the ungrouped
penalty.  It runs in the SparseL1Classifier object with ``set_multinomial(Cn)``: the Cn classes of a model are Cn
neighbouring slots of a chunk of ten fits, floor(10 / Cn) models share a chunk, and the slots behind a chunk's last model
are idle.  This module maps models to slots and back."""
from __future__ import annotations

import time

import numpy as np

from .errorcheck import is_positive_real, penalty_fields, svm_cost_fields
from .solvers import _CG_KEYS, _LOOP_KEYS, _fit_penalties, _lambda_grid, _lambda_vector, _matrix, _options, _pick

_HIST = ("pnorm", "perr", "dnorm", "derr", "objevals")
_REFUSED = ("foldid", "heldout", "obsweights", "groups", "groupweights", "comm")


def slot_map(M, Cn, chunk=10):
    """(the first slot of each of M models of Cn classes, the K slots they need): model j sits in chunk j // P at the
    slots [p*Cn, (p + 1)*Cn) with P = chunk // Cn and p = j % P; the last chunk ends behind its last model"""
    if not 2 <= Cn <= chunk:
        raise ValueError(f"a multinomial model has 2 .. {chunk} classes, not {Cn}")
    per = chunk // Cn
    first = np.array([(j // per) * chunk + (j % per) * Cn for j in range(M)], dtype=np.int64)
    return first, int(first[-1] + Cn)


def model_of_slot(k, Cn, chunk=10):
    """(model, class) of slot k, or None for an idle slot: slot_map's inverse"""
    per = chunk // Cn
    c = k % chunk
    if c >= per * Cn:
        return None
    return (k // chunk) * per + c // Cn, c % Cn


def _refusals(options, who):
    """what the multinomial model does not run, each option named in its ValueError"""
    for key in _REFUSED:
        if options.get(key) is not None:
            raise ValueError(f"options.{key} is not available in {who}: the multinomial model has no folds, groups or "
                             "row sharding")
    for key in ("fast", "convtest", "adaptive"):
        if options.get(key, 0):
            raise ValueError(f"options.{key} is not available in {who}")
    if options.get("relax", 1) != 1:
        raise ValueError(f"options.relax is not available in {who}")
    xs = options.get("xsolve", "auto")
    if not (isinstance(xs, str) and xs.lower() in ("auto", "cg")):
        raise ValueError(f"options.xsolve = {xs!r}: {who} runs the matrix-free x-update ('auto' or 'cg')")
    if options.get("parallel", "none") not in ("none", 0, None):
        raise ValueError(f"options.parallel is not available in {who}")
    if options.get("stopcond", "standard") != "standard":
        raise ValueError(f"options.stopcond: {who} runs the 'standard' stop rule alone")


def _labels(y, m):
    y = np.asarray(y)
    if y.ndim == 2 and 1 in y.shape:
        y = y.reshape(-1)
    if y.ndim != 1:
        raise ValueError("Argument y is not a vector!")
    if y.size != m:
        raise ValueError("The number of rows in argument D do not match size of y!")
    classes, yi = np.unique(y, return_inverse=True)
    if not 2 <= classes.size <= 10:
        raise ValueError(f"y holds {classes.size} distinct classes: the multinomial model takes 2 to 10")
    return classes, yi.astype(np.int64)


def _sparse(D):
    """a dense ndarray goes through scipy.sparse.csr_matrix and runs the same object"""
    from ._lib import is_sparse
    D = _matrix(D, "D", sparse_ok=True)
    if not is_sparse(D):
        import scipy.sparse as sp
        D = sp.csr_matrix(D)
    return D


def _costs(options, yi, Cn):
    """(weights or None, the Cn class weights)"""
    w = svm_cost_fields(dict(weights=options.get("weights")), np.ones(yi.size))
    weights = None if w is None else w["weights"]
    cw = options.get("classweight")
    if cw is None:
        return weights, np.ones(Cn)
    if isinstance(cw, str):
        if cw != "balanced":
            raise ValueError(f"options.classweight = {cw!r}: {Cn} values >= 0 or 'balanced'")
        return weights, yi.size / (Cn * np.bincount(yi, minlength=Cn).astype(np.float64))
    cw = np.asarray(cw, dtype=np.float64).reshape(-1)
    if cw.size != Cn or not np.all(np.isfinite(cw)) or np.any(cw < 0):
        raise ValueError(f"options.classweight is not {Cn} finite values >= 0 (one per class) or 'balanced'")
    return weights, cw


def multinomial_lambda_max(D, y, options=None):
    """The smallest lambda whose multinomial model is x = 0 when every coefficient is penalised:
    C*max over classes c and w_j > 0 of |sum_i c_i*D_ij*(1/Cn - [y_i = c])| / w_j -- at x = 0 every class has
    probability 1/Cn.  With an unpenalised column (w_j = 0) the all-zero model is in general not optimal there."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    D = _matrix(D, "D", sparse_ok=True)
    classes, yi = _labels(y, D.shape[0])
    Cn = classes.size
    weights, cw = _costs(options, yi, Cn)
    c = (np.ones(yi.size) if weights is None else weights) * cw[yi]
    R = (1.0 / Cn - (yi[:, None] == np.arange(Cn)[None, :])) * c[:, None]
    g = np.abs(np.asarray(D.T @ R, dtype=np.float64))
    pw = penalty_fields(dict(l1weights=options.get("l1weights")), D.shape[1])
    if pw is not None:
        live = pw["l1weights"] > 0
        g = g[live] / pw["l1weights"][live, None]
    return is_positive_real(options.get("C", 1.0), "options.C") * (float(g.max()) if g.size else 0.0)


def multinomial_proba(D, xopt):
    """The class probabilities softmax(D*xopt), m x Cn, rows summing to 1; it runs on the host"""
    T = np.asarray(D @ np.asarray(xopt, dtype=np.float64), dtype=np.float64)
    E = np.exp(T - T.max(axis=1, keepdims=True))
    return E / E.sum(axis=1, keepdims=True)


def _run_models(D, y, lams, options, who, t0):
    """M models over one upload of D: the per-model results, in order"""
    from .sparse_l1class import SparseL1Classifier
    _refusals(options, who)
    D = _sparse(D)
    m, n = D.shape
    classes, yi = _labels(y, m)
    Cn = classes.size
    lam = _lambda_vector(lams, "model")
    M = int(lam.size)
    mu, nn, l1weights, _ = _fit_penalties(options, n)
    Cv = is_positive_real(options.get("C", 1.0), "options.C")
    weights, cw = _costs(options, yi, Cn)
    first, K = slot_map(M, Cn, SparseL1Classifier.chunk())
    # the slots: the classes of model j from first[j] on; an idle slot is a valid fit that never runs (labels -1, lambda 0)
    ELL = np.full((m, K), -1.0, order="F")
    lk, rk, nk = np.zeros(K), np.zeros(K), np.zeros(K, dtype=np.int32)
    cost = np.ones((K, 2))
    starts = {}
    for key in ("z0", "u0"):
        if options.get(key) is not None:
            v = np.asarray(options[key], dtype=np.float64)
            if v.shape != (m + n, Cn):
                raise ValueError(f"{key} is not a {m + n} x {Cn} matrix (one column per class: the m rows of D above the "
                                 "n coefficients)")
            starts[key] = (v, np.zeros((m + n, K), order="F"))
    for j in range(M):
        for c in range(Cn):
            k = first[j] + c
            ELL[:, k] = np.where(yi == c, 1.0, -1.0)
            lk[k], rk[k], nk[k] = lam[j], mu, nn
            cost[k, 0] = cw[c]
            for v, full in starts.values():
                full[:, k] = v[:, c]
    obj = SparseL1Classifier(D, ELL, lk, None, rk, nk, l1weights, C=Cv, xsolve=options.get("xsolve", "auto"),
                             device=int(options.get("device", 0)))
    try:
        obj.set_cost(weights, cost)
        obj.set_multinomial(Cn)
        res = obj.results(obj.run(check_every=int(options.get("check_every", 0)),
                                  z0=None if "z0" not in starts else starts["z0"][1],
                                  u0=None if "u0" not in starts else starts["u0"][1],
                                  nodualerror=int(bool(options.get("nodualerror", 0))),
                                  **_pick(options, _LOOP_KEYS + _CG_KEYS)))
    finally:
        obj.close()
    out = []
    for j in range(M):
        k0, k1 = int(first[j]), int(first[j]) + Cn
        steps = int(res["steps"][k0])
        r = {key: np.ascontiguousarray(res[key][:, k0:k1]) for key in ("xopt", "zopt", "uopt")}
        r.update(classes=classes.copy(), steps=steps, lam=float(lam[j]), objopt=float(res["objopt"][k0]))
        r.update({key: np.ascontiguousarray(res[key][:steps, k0]) for key in _HIST if key in res})
        r.update(nnz=res["nnz"], xsolve="cg", cg_iters_total=int(res["cg_iters_total"][k0:k1].sum()),
                 cg_capped_updates=int(res["cg_capped_updates"][k0:k1].sum()), runtime=res["runtime"],
                 solverruntime=time.perf_counter() - t0)
        out.append(r)
    return out


def multinomial(D, y, lam, options=None):
    """results = multinomial(D, y, lam, options): ONE l1 / elastic-net regularised multinomial (softmax) logistic model.

    ``D``: scipy.sparse, any shape; a dense ndarray is converted with ``scipy.sparse.csr_matrix`` and runs the same
    matrix-free object, so the result reads ``xsolve = 'cg'`` either way.  ``y``: m labels of any values; ``classes`` is
    their sorted unique values, 2 to 10 of them.  ``options``: ``C`` (default 1), ``weights`` (m values >= 0), ``classweight``
    (Cn values >= 0 or 'balanced' = m/(Cn*count_c)), ``l1weights`` (n values >= 0 shared by the classes; 0 leaves a
    coefficient unpenalised -- an intercept is a column of ones with weight 0), ``ridge``, ``nonnegative``, ``rho``,
    ``cg_tol`` / ``cg_maxit`` (1e-12 / 200), ``nodualerror``, abstol, reltol, maxiters, domaxiters, objevals, check_every;
    ``z0`` / ``u0`` are (m + n) x Cn.  foldid, heldout, obsweights, groups, comm, xsolve 'inverse' / 'trsv', fast, relax != 1,
    convtest, adaptive, parallel and a stopcond other than 'standard' are refused by name.

    Returns xopt (n x Cn), zopt, uopt ((m + n) x Cn), classes, steps, pnorm, perr, dnorm, derr (unless nodualerror),
    objevals (with options['objevals']), objopt, lam, nnz, cg_iters_total, cg_capped_updates, runtime, solverruntime."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    if not np.isscalar(lam) or not np.isreal(lam):
        raise ValueError("Argument lam is not a nonnegative real number!")
    return _run_models(D, y, [lam], options, "multinomial", time.perf_counter())[0]


def multinomial_path(D, y, lams=None, options=None):
    """results = multinomial_path(D, y, lams, options): M models, one per lambda, in ONE object over one upload of D.
    ``lams``: a list, or a count (None: ``options['nlambda']``, default 6) for a grid log-spaced from
    ``multinomial_lambda_max`` down to ``options['lambda_min_ratio']`` (default 1e-2) times it.  Every model runs to its
    own stop.  Returns xopt (n x Cn x M), zopt, uopt ((m + n) x Cn x M), classes, lams, steps, objopt, cg_iters_total,
    cg_capped_updates (M values each), the histories max(steps) x M (NaN past a model's last step), nnz, runtime,
    solverruntime and ``df`` (M values): the coefficients with any nonzero class in the coefficient block of zopt."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    t0 = time.perf_counter()
    lams = _lambda_grid(options, lams, 6, lambda: multinomial_lambda_max(D, y, options), count_ok=True)
    per = _run_models(D, y, lams, options, "multinomial_path", t0)
    m = per[0]["zopt"].shape[0] - per[0]["xopt"].shape[0]
    steps = np.array([r["steps"] for r in per], dtype=np.int64)
    res = {key: np.stack([r[key] for r in per], axis=2) for key in ("xopt", "zopt", "uopt")}
    for key in _HIST:
        if key in per[0]:
            res[key] = np.full((int(steps.max()), len(per)), np.nan, order="F")
            for j, r in enumerate(per):
                res[key][:steps[j], j] = r[key]
    res.update(classes=per[0]["classes"], lams=np.array([r["lam"] for r in per]), steps=steps,
               objopt=np.array([r["objopt"] for r in per]), nnz=per[0]["nnz"], xsolve="cg",
               cg_iters_total=np.array([r["cg_iters_total"] for r in per], dtype=np.int64),
               cg_capped_updates=np.array([r["cg_capped_updates"] for r in per], dtype=np.int64),
               runtime=per[0]["runtime"], solverruntime=time.perf_counter() - t0)
    res["df"] = np.array([int(np.count_nonzero(np.any(r["zopt"][m:] != 0, axis=1))) for r in per], dtype=np.int64)
    return res
