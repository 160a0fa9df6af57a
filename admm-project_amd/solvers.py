"""Problem solvers with the reference's signatures (/root/reference/solvers/*.m).

Each function is the host half of the corresponding MATLAB solver: validate arguments,
hand the data to ``getproxops`` (which uploads it and builds the cached factor on the
GPU), set the constraint fields of ``options`` exactly as the reference does, call
``admm`` and add ``solverruntime``.  The objective handles the reference installs in
``options.obj`` are realised by device kernels; ``options['obj']`` is therefore a marker.
"""
from __future__ import annotations

import time

import numpy as np

from .api import admm, getproxops
from .errorcheck import LOSS_KEYS, PENALTY_KEYS, SVM_COST_KEYS, class_cost_pair, loss_fields, svm_cost_fields, group_sizes, is_nonnegative_real, is_positive_real, penalty_fields, slicemaker

__all__ = ["lasso", "lasso_multi", "lasso_path", "lasso_cv", "cv_folds", "cv_summary", "grouplasso", "grouplasso_multi", "grouplasso_path", "l1classifier", "l1classifier_multi", "l1classifier_path", "l1classifier_cv", "l1classifier_lambda_max", "elasticnet", "lad", "huberfit", "quantilereg", "robustfit_multi", "quantilereg_multi", "linearsvm", "linearsvm_ovr", "unwrappedadmm", "quadraticprogram", "basispursuit",
           "totalvariation", "totalvariation2d", "model", "linearprogram", "covarianceselection", "covarianceselection_multi",
           "covarianceselection_path", "covarianceselection_lambda_max"]

_ENGINE_OBJ = "<engine-native objective>"


def _matrix(D, name, sparse_ok=False):
    if sparse_ok:  # lasso, grouplasso, elasticnet: a scipy.sparse design matrix goes to the engine as it is
        from ._lib import is_sparse
        if is_sparse(D):
            if len(D.shape) != 2:
                raise ValueError(f"Argument {name} is not a matrix!")
            return D
    D = np.asarray(D, dtype=np.float64)
    if D.ndim != 2:
        raise ValueError(f"Argument {name} is not a matrix!")
    return D


def _colvec(s, name):
    s = np.asarray(s, dtype=np.float64)
    if s.ndim == 2 and 1 in s.shape:
        s = s.reshape(-1)
    if s.ndim != 1:
        raise ValueError(f"Argument {name} is not a vector!")
    return s


def _engine_args(options, args, **more):
    args.update(more)
    for key in ("xsolve", "device", "comm", "cg_tol", "cg_maxit", "objgram"):
        if key in options:
            args[key] = options[key]
    return args


def _options(options, message, optional=False):
    """a copy of the caller's options (``optional``: None stands for an empty dict); ``message``: the solver's TypeError"""
    if optional and options is None:
        options = {}
    if not isinstance(options, dict):
        raise TypeError(message)
    return dict(options)


# ---- shared by the multi-fit solvers (K runs over one D: DESIGN.md q36-q39)
_LOOP_KEYS = ("rho", "abstol", "reltol", "maxiters", "domaxiters", "objevals")
_CG_KEYS = ("cg_tol", "cg_maxit")


def _pick(options, keys):
    return {k: options[k] for k in keys if k in options}


def _response_matrix(S, m):
    """the responses as a matrix of m rows: a vector stands for one column"""
    S = np.asarray(S, dtype=np.float64)
    if S.ndim == 1:
        S = S.reshape(-1, 1)
    if S.ndim != 2:
        raise ValueError("Argument S is neither a vector nor a matrix!")
    if S.shape[0] != m:
        raise ValueError("The number of rows in argument D do not match size of S!")
    return S


def _response_columns(S, K):
    if S.shape[1] not in (1, K):
        raise ValueError(f"S has {S.shape[1]} columns for {K} fits: one shared response or one column per fit")
    return np.asfortranarray(S)


def _start_matrices(options, rows_by_key, K, unit, default=None):
    """options.x0 / z0 / u0 as rows x K matrices, one column per ``unit``.  Without ``default`` a start that is missing
    or None is left out (zeros); with it, a missing one is ``default((rows, K))``"""
    starts = {}
    for key, rows in rows_by_key.items():
        if key in options if default else options.get(key) is not None:
            v = np.asarray(options[key], dtype=np.float64)
            if v.shape != (rows, K):
                raise ValueError(f"options.{key} is not a {rows} x {K} matrix (one column per {unit})!")
        elif default:
            v = default((rows, K))
        else:
            continue
        starts[key] = np.asfortranarray(v)
    return starts


def _start_columns(options, rows_by_key, default=None):
    """the K = 1 case from vectors: options.x0 / z0 / u0 as rows x 1 matrices"""
    starts = {}
    for key, rows in rows_by_key.items():
        if key in options if default else options.get(key) is not None:
            v = _colvec(options[key], key)
        elif default:
            v = default(rows)
        else:
            continue
        if v.size != rows:
            raise ValueError(f"options.{key} does not have {rows} entries!")
        starts[key] = np.asfortranarray(v.reshape(rows, 1))
    return starts


def _sparse_refusals(options, who, also=(), stopcond=False, observations=False, folds=False):
    """the options no sparse multi-fit object runs, each named in its ValueError; ``also``: keys
    refused beside comm, ``stopcond``: the object runs the 'standard' stop rule alone, ``observations``: the object takes
    obsweights / foldid / heldout (the multi-lasso: q46), ``folds``: it takes foldid / heldout and has observation
    weights under a name of its own (the classifier's ``weights``: q47)"""
    if folds:
        if options.get("obsweights") is not None:
            raise ValueError(f"options.obsweights is not available in {who}: the classifier's observation weights are "
                             "options.weights")
    elif not observations:
        _no_observations(options, who)
    for key in ("fast", "convtest", "adaptive"):
        if options.get(key, 0):
            raise ValueError(f"options.{key} is not available in {who} on a sparse D")
    if options.get("relax", 1) != 1:
        raise ValueError(f"options.relax is not available in {who} on a sparse D")
    xs = options.get("xsolve", "auto")
    if not (isinstance(xs, str) and xs.lower() in ("auto", "cg")):
        raise ValueError(f"options.xsolve = {xs!r}: {who} on a sparse D runs the matrix-free x-update ('auto' or 'cg')")
    for key in also + ("comm",):
        if options.get(key) is not None:
            raise ValueError(f"options.{key} is not available in {who} on a sparse D")
    if options.get("parallel", "none") not in ("none", 0, None):
        raise ValueError(f"options.parallel is not available in {who} on a sparse D")
    if stopcond and options.get("stopcond", "standard") != "standard":
        raise ValueError(f"options.stopcond: {who} on a sparse D runs the 'standard' stop rule alone")


def _run_and_close(obj, prepare=None, finish=None, **run):
    """``prepare``: a setter ``f(obj)`` (the weights or costs, if any) or a list of them, applied in order, None standing
    for none; then one run and the owner's results (engine._MultiOwner.results), which ``finish(obj, results)`` may add
    to while the owner lives; the owner is closed in any case"""
    try:
        for setter in prepare if isinstance(prepare, list) else [prepare]:
            if setter is not None:
                setter(obj)
        res = obj.results(obj.run(**run))
        if finish is not None:
            finish(obj, res)
        return res
    finally:
        obj.close()


_OBSERVATION_KEYS = ("obsweights", "foldid", "heldout")


def _no_observations(options, who):
    """observation weights and held-out folds live on the sparse multi-lasso alone: every other
    multi-fit family names the option it refuses"""
    for key in _OBSERVATION_KEYS:
        if options.get(key) is not None:
            raise ValueError(f"options.{key} is not available in {who}: observation weights and held-out folds are "
                             "lasso_multi's, on a scipy.sparse D")


def _stack_fits(per, hist_keys):
    """the results of K single-fit runs side by side, as a multi-fit owner returns them: a column per fit, the
    histories NaN past a fit's last step"""
    steps = np.array([r["steps"] for r in per], dtype=np.int64)
    res = {key: np.asfortranarray(np.stack([np.asarray(r[key]).reshape(-1) for r in per], axis=1))
           for key in ("xopt", "zopt", "uopt")}
    for key in hist_keys:
        if all(key in r for r in per):
            res[key] = np.full((int(steps.max()), len(per)), np.nan, order="F")
            for c, r in enumerate(per):
                res[key][:steps[c], c] = np.asarray(r[key])[:steps[c]]
    res["steps"] = steps
    res["objopt"] = np.array([r.get("objopt", np.nan) for r in per], dtype=np.float64)
    res["runtime"] = float(sum(r["runtime"] for r in per))
    return res


def _drop_fit_axis(res, hist_keys):
    """a K = 1 result as the single-fit solvers return it: vectors, and Python scalars for steps, objopt and the CG
    counters"""
    for key in ("xopt", "zopt", "uopt") + hist_keys:
        if key in res:
            res[key] = np.ascontiguousarray(res[key][:, 0])
    for key in ("steps", "cg_iters_total", "cg_capped_updates"):
        res[key] = int(res[key][0])
    res["objopt"] = float(res["objopt"][0])
    return res


def lasso(D, s, lam, options=None):
    """results = lasso(D, s, lambda, options)   (solvers/lasso.m:77-245)

    minimise 1/2*||D*x - s||_2^2 + lambda*||x||_1.  Setup on the device: Dts = D'*s,
    L = chol(D'*D + rho*I) (tall) or chol(D*D'/rho + I) (fat) (lasso.m:160-176).

    ``D`` may be any ``scipy.sparse`` matrix or array (engine-side extension): it is converted to
    canonical CSC and stays sparse on the device; the x-update is then the matrix-free CG of ``xsolve = 'cg'`` with two
    sparse products per inner iteration (tall or fat D), ``results['xsolve']`` reads 'cg' and ``results['nnz']`` is the
    stored count.  ``xsolve = 'trsv' | 'inverse'``, ``args.L``, ``options['parallel']`` and ``options['comm']`` are
    refused by the engine.

    Engine-side extension: ``options['l1weights']`` (n values w_i >= 0: lambda*sum_i w_i*|x_i|),
    ``options['ridge']`` (mu >= 0: + mu/2*||x||^2, the elastic net) and ``options['nonnegative']`` (1: x >= 0) change
    the z-update alone; the serial solver only.
    """
    options = _options(options, "Given options is not a struct! At least pass empty struct!")
    t0 = time.perf_counter()
    lam = is_nonnegative_real(lam, "lambda")
    D = _matrix(D, "D", sparse_ok=True)
    s = _colvec(s, "s")
    rho = is_positive_real(options["rho"], "options.rho") if "rho" in options else 1.0
    m, n = D.shape
    if s.size != m:
        raise ValueError("The number of rows in argument D do not match size of s!")
    penalty = penalty_fields({k: options.pop(k, None) for k in PENALTY_KEYS if k != "l1"}, n)
    if penalty is not None and (options.get("parallel", "none") in ("both", "zming", "xminf") or "comm" in options):
        raise ValueError("l1weights / ridge / nonnegative have no consensus or row-sharded form: options.parallel / "
                         "options.comm")
    if options.get("parallel", "none") in ("both", "zming", "xminf"):  # lasso.m:144-156, 193-224
        # consensus lasso: row slices each with their own x_k, u_k and cached factor.  `workers`
        # stands for gcp().NumWorkers (lasso.m:203-207); with options['comm'] D, s are this rank's rows
        # and the slices given here are this rank's local slices.
        options["parallel"] = "none"
        options["stopcond"] = "both"
        slices = np.atleast_1d(options.get("slices", 0))[0]  # lasso.m:197 takes only slices(1)
        workers = int(options.get("workers", 1 if "comm" in options else 8))
        args = _engine_args(options, dict(D=D, s=s, rho=rho, parallel=1, slices=slicemaker(slices, workers, m)))
        args["lambda"] = lam
        minx, minz, extra = getproxops("LASSO", args)
        options["altu"] = extra["altu"]  # lasso.m:222-223
        options["specialnorms"] = extra["specialnorms"]
    else:
        args = _engine_args(options, dict(D=D, s=s, m=m, n=n, parallel=0, rho=rho), **(penalty or {}))
        args["lambda"] = lam
        minx, minz, _ = getproxops("LASSO", args)
    options["obj"] = _ENGINE_OBJ  # lasso.m:227  0.5*sum((D*x - s).^2) + lambda*norm(z,1)  (+ the penalty family's terms)
    options.update(A=1, At=1, m=n, nA=n, nB=n, B=-1, c=0, parallel="none")  # lasso.m:232-239
    results = admm(minx, minz, options)
    results["solverruntime"] = time.perf_counter() - t0
    return results


def grouplasso(D, s, lam, groups, options=None):
    """results = grouplasso(D, s, lambda, groups, options): an engine-side extension in the shape of lasso().

    minimise 1/2*||D*x - s||_2^2 + lambda*sum_g w_g*||x_g||_2 over contiguous groups of coefficients: ``groups`` holds
    their sizes (integers >= 1 that sum to the columns of D), ``options['groupweights']`` the optional w_g >= 0
    (default 1; sqrt(p_g) is the caller's choice).  The x-update and every option are the lasso's; the z-update is the
    block soft threshold z_g = v_g*max(0, 1 - (lambda*w_g/rho)/||v_g||) on the device (Boyd et al. 6.4.2).
    ``options['l1']`` > 0 adds l1*sum_i w_i*|x_i| (the sparse-group lasso); ``options['l1weights']``, ``['ridge']`` and
    ``['nonnegative']`` are lasso()'s."""
    options = _options(options, "Given options is not a struct! At least pass empty struct!")
    t0 = time.perf_counter()
    lam = is_nonnegative_real(lam, "lambda")
    D = _matrix(D, "D", sparse_ok=True)
    s = _colvec(s, "s")
    rho = is_positive_real(options["rho"], "options.rho") if "rho" in options else 1.0
    m, n = D.shape
    if s.size != m:
        raise ValueError("The number of rows in argument D do not match size of s!")
    sizes, weights = group_sizes(groups, options.pop("groupweights", None), n)
    penalty = penalty_fields({k: options.pop(k, None) for k in PENALTY_KEYS}, n)
    if options.get("parallel", "none") in ("both", "zming", "xminf") or "comm" in options:
        raise ValueError("grouplasso has no consensus or row-sharded form: options.parallel / options.comm")
    args = _engine_args(options, dict(D=D, s=s, m=m, n=n, parallel=0, rho=rho, groups=sizes), **(penalty or {}))
    if weights is not None:
        args["groupweights"] = weights
    args["lambda"] = lam
    minx, minz, _ = getproxops("LASSO", args)
    options["obj"] = _ENGINE_OBJ  # 0.5*sum((D*x - s).^2) + lambda*sum_g w_g*norm(z_g)
    options.update(A=1, At=1, m=n, nA=n, nB=n, B=-1, c=0, parallel="none")
    results = admm(minx, minz, options)
    results["solverruntime"] = time.perf_counter() - t0
    return results


def elasticnet(D, s, lam, ridge, options=None):
    """results = elasticnet(D, s, lambda, ridge, options): minimise 1/2*||D*x - s||_2^2 + lambda*||x||_1 +
    ridge/2*||x||_2^2 -- lasso() with options['ridge'].  The ridge term lives in the z-update
    (z = rho/(rho + ridge) * soft threshold), so the cached factor of the x-update is the lasso's whatever ridge is."""
    if not isinstance(options, dict):
        raise TypeError("Given options is not a struct! At least pass empty struct!")
    return lasso(D, s, lam, dict(options, ridge=ridge))


def _per_fit(value, K, name, check):
    """a scalar (for every fit) or K values, each passed through ``check`` (a penalty_fields field); messages name the fit"""
    vals = [value] * K if np.isscalar(value) or isinstance(value, (bool, np.bool_)) else list(np.asarray(value).reshape(-1))
    if len(vals) != K:
        raise ValueError(f"{name} has {len(vals)} entries for {K} fits")
    out = []
    for k, v in enumerate(vals):
        try:
            out.append(check(v.item() if isinstance(v, np.generic) else v))
        except ValueError as e:
            raise ValueError(f"fit {k}: {e}") from None
    return out


def _lambda_max(D, S, w, obsw=None):
    """per column of S the smallest lambda whose lasso solution is x = 0: max over w_i > 0 of |(D's)_i| / w_i; under
    observation weights ``obsw`` the product is D'(obsw o s)"""
    if obsw is not None:
        S = np.asarray(S, dtype=np.float64) * (obsw if np.ndim(S) == 1 else obsw[:, None])
    g = np.abs(np.asarray(D.T @ S, dtype=np.float64)).reshape(D.shape[1], -1)
    if w is not None:
        live = w > 0
        g = g[live] / w[live][:, None]
    return g.max(axis=0) if g.size else np.zeros(S.shape[1] if S.ndim == 2 else 1)


def _lambda_vector(lams, unit="fit", zero_ok=True):
    """lams as a vector of at least one value, each finite and >= 0 (> 0 without ``zero_ok``); ``unit`` names what a
    value belongs to in the message, None leaves the values to the runner behind the caller"""
    lam = np.asarray(lams, dtype=np.float64).reshape(-1)
    if lam.size < 1:
        raise ValueError("lams must hold at least one lambda")
    for k, v in enumerate(lam if unit is not None else ()):
        if not np.isfinite(v) or not (v >= 0 if zero_ok else v > 0):
            raise ValueError(f"{unit} {k}: lambda is not a {'nonnegative' if zero_ok else 'positive'} real number")
    return lam


def _lambda_grid(options, lams, default_n, lmax, count_ok=False):
    """the lambdas of a path: ``lams`` as given, or -- for None, and with ``count_ok`` for a scalar, which then is the
    count -- options.nlambda values (default ``default_n``; an integer >= 1, not a bool) log-spaced from ``lmax()`` down
    to options.lambda_min_ratio (default 1e-2) times it.  The two options are popped in every case; ``lmax`` is called
    once both have passed"""
    nlambda = options.pop("nlambda", None)
    ratio = options.pop("lambda_min_ratio", 1e-2)
    if lams is not None and not (count_ok and np.isscalar(lams)):
        return lams
    nlambda = lams if lams is not None else default_n if nlambda is None else nlambda
    if isinstance(nlambda, bool) or not isinstance(nlambda, (int, np.integer)) or nlambda < 1:
        raise ValueError("options.nlambda must be an integer >= 1")
    if not np.isscalar(ratio) or not np.isreal(ratio) or not 0.0 < ratio <= 1.0:
        raise ValueError("options.lambda_min_ratio must lie in (0, 1]")
    top = float(lmax())
    return top * np.logspace(0.0, np.log10(float(ratio)), int(nlambda)) if nlambda > 1 else np.array([top])


def _lasso_grid(D, s, lams, options, lmax=None):
    """lasso_path's ``_lambda_grid`` of 10 values from the lasso's lambda_max under options.l1weights and
    options.obsweights; ``lmax()``: another lambda_max (grouplasso_path)"""
    if lams is None and s.size != D.shape[0]:
        raise ValueError("The number of rows in argument D do not match size of s!")

    def lasso_lmax():
        pw = penalty_fields(dict(l1weights=options.get("l1weights")), D.shape[1])
        obsw = options.get("obsweights")
        if obsw is not None:
            from .sparse_lasso import observation_arrays
            obsw = observation_arrays(obsw, None, None, D.shape[0], 1)[0]
        return _lambda_max(D, s.reshape(-1, 1), None if pw is None else pw["l1weights"], obsw)[0]

    return _lambda_grid(options, lams, 10, lmax or lasso_lmax)


def _fit_penalties(options, n, K=None, groups=None):
    """(ridge, nonnegative, l1weights, None | (group sizes, group weights, l1)): ridge, nonnegative and, beside ``groups``,
    l1 are K values out of a scalar or K values (``K = None``: one value, the multinomial model), the l1 weights are
    shared; options.rho, where given, is checked to be positive"""
    def field(key, default):
        check = lambda v: penalty_fields({key: v}, n)[key]
        return check(options.get(key, default)) if K is None else _per_fit(options.get(key, default), K, key, check)

    ridge, nonneg = field("ridge", 0.0), field("nonnegative", 0)
    pw = penalty_fields(dict(l1weights=options.get("l1weights")), n)
    if "rho" in options:
        is_positive_real(options["rho"], "options.rho")
    grouped = None if groups is None else group_sizes(groups, options.get("groupweights"), n) + (field("l1", 0.0),)
    return ridge, nonneg, None if pw is None else pw["l1weights"], grouped


def _run_multi_lasso(D, S, lams, options, who, sparse, t0, groups=None):
    """the body of lasso_multi (sparse) and lasso_multi_dense behind their refusal of the other kind of D, and of
    grouplasso_multi on either: the refusals, the fits, the owner, one run.  ``groups``: the sizes of grouplasso_multi;
    options.groupweights and options.l1 are read beside them alone, and the result carries ``groups``"""
    if sparse:
        _sparse_refusals(options, who, stopcond=True, observations=True)
    else:
        _dense_multi_refusals(options, who)
    D = _matrix(D, "D", sparse_ok=sparse)
    m, n = D.shape
    S = _response_matrix(S, m)
    lam = _lambda_vector(lams)
    K = int(lam.size)
    S = _response_columns(S, K)
    ridge, nonneg, w, grouped = _fit_penalties(options, n, K, groups)
    starts = _start_matrices(options, dict(x0=n, z0=n, u0=n), K, "fit")
    prepare, finish = [None if grouped is None else lambda obj: obj.set_groups(*grouped)], None
    if sparse and any(options.get(key) is not None for key in _OBSERVATION_KEYS):
        from .sparse_lasso import observation_arrays
        obs = observation_arrays(options.get("obsweights"), options.get("foldid"), options.get("heldout"), m, K)
        prepare.append(lambda obj: obj.set_observations(*obs[:3]))

        def finish(obj, res):
            res["heldout_sse"], res["heldout_weight"] = obj.heldout()
    if not sparse and m < n:
        raise ValueError(f"{who} needs m >= n: the fat lasso's x-update (two dense products per fit) stays with lasso, "
                         "one call per fit")
    run = dict(check_every=int(options.get("check_every", 0)), z0=starts.get("z0"), u0=starts.get("u0"),
               nodualerror=int(bool(options.get("nodualerror", 0))))
    if sparse:
        from .sparse_lasso import SparseLassoMulti
        obj = SparseLassoMulti(D, S, lam, ridge, nonneg, w, device=int(options.get("device", 0)))
        run.update(_pick(options, _LOOP_KEYS + _CG_KEYS))
    else:
        from .lasso_multi import LassoMulti
        obj = LassoMulti(D, S, lam, ridge, nonneg, w, rho=float(options.get("rho", 1.0)),
                         xsolve=options.get("xsolve", "auto"), device=int(options.get("device", 0)))
        run.update(_pick(options, _LOOP_KEYS))
    res = _run_and_close(obj, prepare, finish, **run)
    res["lams"] = lam.copy()
    if grouped is not None:
        res["groups"] = grouped[0].copy()
    res["solverruntime"] = time.perf_counter() - t0
    return res


def lasso_multi(D, S, lams, options=None):
    """results = lasso_multi(D, S, lams, options): K lasso fits over ONE sparse design matrix in one run
    -- a regularisation path, a cross-validation grid, or one D against several response columns:

        minimise 1/2*||D*x - s_k||^2 + lambda_k*sum_i w_i*|x_i| + ridge_k/2*||x||^2   (x >= 0 where nonnegative_k)

    ``D``: any ``scipy.sparse`` matrix or array; a dense D raises ValueError (``lasso_multi_dense`` is its form).  ``S``: a vector
    or m x 1 (shared by all fits) or m x K (one column per fit).  ``lams``: the K values lambda_k >= 0.
    ``options['ridge']`` and ``options['nonnegative']`` are scalars or K values, ``options['l1weights']`` (n values >= 0)
    is shared by all fits.  rho, abstol, reltol, maxiters, domaxiters, objevals and check_every apply to every fit;
    ``z0`` / ``u0`` are n x K (default zeros), x0 (n x K) is checked and never read; ``nodualerror`` (default 0: the
    reference lasso's stop rule on both residuals) set to 1 stops on the primal residual alone; ``cg_tol`` / ``cg_maxit``
    (1e-12 / 200) bound a solve.  Every x-update is conjugate gradients on (D'D + rho*I) x = D's_k + rho*(z - u), all fits
    in lock-step over one sparse product.

    Returns xopt, zopt, uopt (n x K), steps (K), pnorm / perr (max(steps) x K, NaN past a fit's last step), dnorm / derr
    unless nodualerror = 1, objevals with options['objevals'], objopt (K), runtime, solverruntime, chunk, lams,
    ``xsolve = 'cg'``, ``nnz``, ``cg_iters_total`` and ``cg_capped_updates`` (K values each).  fast, convtest, relax,
    adaptive, an xsolve other than 'auto' / 'cg', comm, parallel and a stopcond other than 'standard' are refused by
    name.

    Observations: ``options['obsweights']`` (m values >= 0 shared by all fits), ``options['foldid']`` (m
    integer fold ids >= 0) and ``options['heldout']`` (K integers: the fold fit k leaves out, -1 for none) turn the fit
    term of fit k into 1/2*sum_i omega_ik*(d_i'x - s_ik)^2 with omega_ik = obsweights_i * [foldid_i != heldout_k].  The
    result then carries ``heldout_sse`` and ``heldout_weight`` (K values each): the weighted squared error of zopt on
    the rows the fit held out, and their total weight.  ``lasso_cv`` builds a cross-validation out of them."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    t0 = time.perf_counter()
    from ._lib import is_sparse
    if not is_sparse(D):
        raise ValueError("lasso_multi runs on a scipy.sparse D: call lasso per fit on a dense design matrix")
    return _run_multi_lasso(D, S, lams, options, "lasso_multi", True, t0)


def lasso_path(D, s, lams=None, options=None):
    """results = lasso_path(D, s, lams, options): the lasso's regularisation path on a sparse D, every lambda side by side
    in one run of ``lasso_multi``.  ``lams = None``: ``options['nlambda']`` values (default: the chunk of
    the sparse product, 10), log-spaced from lambda_max = max over w_i > 0 of |(D's)_i| / w_i -- the smallest lambda whose
    solution is x = 0 -- down to ``options['lambda_min_ratio']`` * lambda_max (default 1e-2).  Returns lasso_multi's
    fields plus ``df``, the number of nonzeros of each zopt column.  A dense D raises ValueError: ``lasso_path_dense``.
    Under ``options['obsweights']`` lambda_max is taken from D'(obsweights o s)."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    from ._lib import is_sparse
    if not is_sparse(D):
        raise ValueError("lasso_path runs on a scipy.sparse D: call lasso per lambda on a dense design matrix")
    s = _colvec(s, "s")
    res = lasso_multi(D, s, _lasso_grid(D, s, lams, options), options)  # (10 = kSpmmChunk: one pass over D per product)
    res["df"] = np.count_nonzero(res["zopt"], axis=0).astype(np.int64)
    return res


def cv_folds(m, nfolds, seed=0):
    """the default fold of each of m observations: ``np.random.default_rng(seed).permutation(m) % nfolds``"""
    return (np.random.default_rng(seed).permutation(int(m)) % int(nfolds)).astype(np.int64)


def cv_summary(sse, weight, lams):
    """The cross-validation curve from the held-out sums.  ``sse`` and ``weight`` are F x L (fold f, lambda
    l): the weighted squared error on the rows fold f held out and their total weight; ``lams`` the L values.  Returns

        cvm        L values: sum_f sse_fl / sum_f weight_fl, the weighted mean of the folds' own errors e_fl = sse_fl / weight_fl
        cvsd       the weighted standard error over folds: sqrt(sum_f weight_fl*(e_fl - cvm_l)^2 / sum_f weight_fl / (F - 1))
                   (NaN for F = 1)
        index_min  where cvm is smallest; among equal values the largest lambda
        lam_min    lams[index_min]
        index_1se  the largest lambda with cvm <= cvm[index_min] + cvsd[index_min] (index_min itself when cvsd is NaN)
        lam_1se    lams[index_1se]

    A fold of zero weight takes no part in either sum."""
    sse = np.atleast_2d(np.asarray(sse, dtype=np.float64))
    weight = np.atleast_2d(np.asarray(weight, dtype=np.float64))
    lams = np.asarray(lams, dtype=np.float64).reshape(-1)
    if sse.shape != weight.shape or sse.shape[1] != lams.size:
        raise ValueError(f"sse {sse.shape} and weight {weight.shape} must both be folds x {lams.size} lambdas")
    F = sse.shape[0]
    wsum = weight.sum(axis=0)
    cvm = sse.sum(axis=0) / wsum
    live = weight > 0
    e = np.divide(sse, weight, out=np.zeros_like(sse), where=live)
    dev = np.where(live, weight * (e - cvm[None, :]) ** 2, 0.0)
    cvsd = np.sqrt(dev.sum(axis=0) / wsum / (F - 1)) if F > 1 else np.full(lams.size, np.nan)

    def largest_lambda(mask):
        idx = np.flatnonzero(mask)
        return int(idx[np.argmax(lams[idx])])

    index_min = largest_lambda(cvm == np.min(cvm))
    bar = cvm[index_min] + cvsd[index_min]
    index_1se = largest_lambda(cvm <= bar) if np.isfinite(bar) else index_min
    return dict(cvm=cvm, cvsd=cvsd, index_min=index_min, lam_min=float(lams[index_min]), index_1se=index_1se,
                lam_1se=float(lams[index_1se]))


def _cv_folds(options, who, m, y, name):
    """(F, foldid, scale) of a cross-validation of ``who`` over m observations: options.nfolds, seed and scale_lambda are
    popped, options.heldout is refused, the response ``y`` (``name`` in the message) has m entries, and foldid is
    options.foldid with every id in [0, F), or ``cv_folds``' default"""
    F = options.pop("nfolds", 5)
    if isinstance(F, bool) or not isinstance(F, (int, np.integer)) or F < 2:
        raise ValueError("options.nfolds must be an integer >= 2")
    F = int(F)
    seed = options.pop("seed", 0)
    scale = bool(options.pop("scale_lambda", 1))
    if options.get("heldout") is not None:
        raise ValueError(f"options.heldout is {who}'s own to set: give options.foldid")
    options.pop("heldout", None)
    if y.size != m:
        raise ValueError(f"The number of rows in argument D do not match size of {name}!")
    if options.get("foldid") is None:
        return F, cv_folds(m, F, seed), scale
    from .sparse_lasso import observation_arrays
    foldid = observation_arrays(None, options["foldid"], None, m, 1)[1].astype(np.int64)
    if foldid.min() < 0 or foldid.max() >= F:
        raise ValueError(f"options.foldid: every fold id must lie in [0, nfolds = {F})")
    return F, foldid, scale


def _cv_layout(options, lams, foldid, F, scale, w, wname, per_lambda, start_rows):
    """The (F + 1)*L fits of a cross-validation over the L ``lams``, written into ``options``: fit f*L + l leaves fold f
    out at lambda_l, fits F*L + l see every row.  Sets foldid and heldout, tiles the ``per_lambda`` options given as L
    values and the starts (``start_rows``: the rows of each, L columns) F + 1 times, and returns fold_lams (F x L):
    lambda_l times the training weight of fold f over the total of the observation weights ``w`` (options.``wname``),
    or lambda_l itself without ``scale``.  The lambdas of the run are fold_lams row by row, then lams"""
    L = int(lams.size)
    total = float(w.sum())
    if not total > 0.0:
        raise ValueError(f"options.{wname}: the total weight must be positive")
    train = np.array([total - float(w[foldid == f].sum()) for f in range(F)])
    fold_lams = (train / total if scale else np.ones(F))[:, None] * lams[None, :]
    options["foldid"] = foldid
    options["heldout"] = np.concatenate([np.repeat(np.arange(F), L), np.full(L, -1)])
    for key in per_lambda:  # scalars, or L values for every fold alike
        if key in options and not (np.isscalar(options[key]) or isinstance(options[key], (bool, np.bool_))):
            v = np.asarray(options[key]).reshape(-1)
            if v.size != L:
                raise ValueError(f"{key} has {v.size} entries for {L} lambdas")
            options[key] = np.tile(v, F + 1)
    for key, rows in start_rows.items():
        if options.get(key) is not None:
            v = np.asarray(options[key], dtype=np.float64)
            if v.shape != (rows, L):
                raise ValueError(f"options.{key} is not a {rows} x {L} matrix (one column per lambda)!")
            options[key] = np.asfortranarray(np.tile(v, (1, F + 1)))
    return fold_lams


def _cv_results(res, lams, foldid, fold_lams, held_keys, error_key, row0=0, sizes=None, **first):
    """the result of ``_cv_layout``'s run cut back into the F x L fold blocks (``held_keys``: the held-out sums, the
    weight last; fold_steps) and the L full-data fits; ``cv_summary`` of ``error_key``; df (and, with the group
    ``sizes``, groups and df_groups) of the coefficient block of zopt, which starts at ``row0``"""
    F, L = fold_lams.shape
    full = slice(F * L, (F + 1) * L)
    held = {key: res[key][:F * L].reshape(F, L) for key in held_keys}
    out = dict(lams=lams.copy(), foldid=foldid, **first, **cv_summary(held[error_key], held[held_keys[-1]], lams))
    for key in ("xopt", "zopt", "uopt"):
        out[key] = np.asfortranarray(res[key][:, full])
    out["df"] = np.count_nonzero(out["zopt"][row0:], axis=0).astype(np.int64)
    if sizes is not None:
        out.update(groups=sizes.copy(), df_groups=_df_groups(out["zopt"][row0:], sizes))
    out.update(steps=res["steps"][full], objopt=res["objopt"][full], fold_steps=res["steps"][:F * L].reshape(F, L),
               fold_lams=fold_lams, **held, nnz=res["nnz"], cg_iters_total=res["cg_iters_total"],
               cg_capped_updates=res["cg_capped_updates"], chunk=res["chunk"], runtime=res["runtime"])
    return out


def lasso_cv(D, s, lams=None, options=None):
    """results = lasso_cv(D, s, lams, options): F-fold cross-validation of the lasso's regularisation path on a sparse D,
    every fold fit and every full-data fit side by side in ONE run of ``lasso_multi`` over one upload of D (DESIGN.md
    q46).  ``lams = None``: ``lasso_path``'s grid (``nlambda``, default 10; ``lambda_min_ratio``, default 1e-2;
    lambda_max under ``obsweights`` from D'(obsweights o s)).  With L lambdas and F = ``options['nfolds']`` (default 5)
    the object holds (F + 1)*L fits: fit f*L + l leaves fold f out at lambda_l, fits F*L + l see every row.

    ``options['foldid']``: m fold ids in [0, nfolds); absent: ``cv_folds(m, nfolds, options.get('seed', 0))``.  A fold fit
    runs at lambda_l * (training weight of fold f / total weight): one lambda sequence on the per-observation scale, as
    glmnet poses it, written for this unnormalised objective; ``options['scale_lambda'] = 0`` runs every fold at
    lambda_l itself.  ``obsweights``, ``l1weights``, ``ridge`` and ``nonnegative`` (scalars or L values), and the loop /
    CG options are lasso_multi's; ``z0`` / ``u0`` (n x L) start every fold alike.

    Returns lams, foldid, ``cv_summary``'s cvm, cvsd, index_min, lam_min, index_1se, lam_1se; xopt, zopt, uopt (n x L),
    df, steps, objopt of the full-data fits; fold_steps, fold_lams, heldout_sse, heldout_weight (F x L); nnz,
    cg_iters_total and cg_capped_updates over all (F + 1)*L fits, runtime and solverruntime."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    t0 = time.perf_counter()
    from ._lib import is_sparse
    if not is_sparse(D):
        raise ValueError("lasso_cv runs on a scipy.sparse D")
    s = _colvec(s, "s")
    m, n = D.shape
    F, foldid, scale = _cv_folds(options, "lasso_cv", m, s, "s")
    from .sparse_lasso import observation_arrays
    obsw = observation_arrays(options.get("obsweights"), None, None, m, 1)[0]
    lams = _lambda_vector(_lasso_grid(D, s, lams, options), None)
    fold_lams = _cv_layout(options, lams, foldid, F, scale, np.ones(m) if obsw is None else obsw, "obsweights",
                           ("ridge", "nonnegative"), dict(x0=n, z0=n, u0=n))
    res = lasso_multi(D, s, np.concatenate([fold_lams.reshape(-1), lams]), options)
    out = _cv_results(res, lams, foldid, fold_lams, ("heldout_sse", "heldout_weight"), "heldout_sse")
    out["solverruntime"] = time.perf_counter() - t0
    return out


def _dense_multi_refusals(options, who):
    """the options the dense multi-lasso does not run, each named in its ValueError"""
    for key in ("fast", "convtest", "adaptive"):
        if options.get(key, 0):
            raise ValueError(f"options.{key} is not available in {who}")
    if options.get("relax", 1) != 1:
        raise ValueError(f"options.relax is not available in {who}")
    from .lasso_multi import xsolve_code
    xsolve_code(options.get("xsolve", "auto"))
    _no_observations(options, who)  # (one Gram matrix serves all fits of a dense object: q46)
    if options.get("comm") is not None:
        raise ValueError(f"options.comm is not available in {who}")
    if options.get("parallel", "none") not in ("none", 0, None):
        raise ValueError(f"options.parallel is not available in {who}")
    if options.get("stopcond", "standard") != "standard":
        raise ValueError(f"options.stopcond: {who} runs the 'standard' stop rule alone")


def lasso_multi_dense(D, S, lams, options=None):
    """results = lasso_multi_dense(D, S, lams, options): ``lasso_multi``'s K fits on a DENSE design matrix, m >= n, in one
    run over one cached inverse.  The arguments, ``ridge`` / ``nonnegative`` / ``l1weights``, ``z0`` /
    ``u0`` (n x K), ``nodualerror`` and the loop options are lasso_multi's; ``options['rho']`` (default 1) is fixed when
    the factor of D'D + rho*I is built; ``options['xsolve']`` is 'auto' (the engine's accuracy probe decides), 'inverse'
    (the explicit inverse, read once per chunk of fits) or 'trsv' (K pairs of triangular solves).

    Returns lasso_multi's fields without nnz and the CG counters; ``xsolve`` reads 'inverse' or 'trsv'.  A scipy.sparse D
    raises ValueError (``lasso_multi`` is its form), and so does m < n: the fat lasso stays with ``lasso``."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    t0 = time.perf_counter()
    from ._lib import is_sparse
    if is_sparse(D):
        raise ValueError("lasso_multi_dense runs on a dense D: call lasso_multi on a scipy.sparse design matrix")
    return _run_multi_lasso(D, S, lams, options, "lasso_multi_dense", False, t0)


def lasso_path_dense(D, s, lams=None, options=None):
    """results = lasso_path_dense(D, s, lams, options): ``lasso_path`` on a dense D through ``lasso_multi_dense`` -- the
    same automatic grid (``nlambda``, default 10 = one chunk of the product; ``lambda_min_ratio``, default 1e-2; the same
    lambda_max) and the same ``df``."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    from ._lib import is_sparse
    if is_sparse(D):
        raise ValueError("lasso_path_dense runs on a dense D: call lasso_path (lasso_multi) on a scipy.sparse design matrix")
    D = _matrix(D, "D")
    s = _colvec(s, "s")
    res = lasso_multi_dense(D, s, _lasso_grid(D, s, lams, options), options)
    res["df"] = np.count_nonzero(res["zopt"], axis=0).astype(np.int64)
    return res


# ---- sparse linear classifiers: the lasso's penalties on the linear SVM's losses
_L1C_HIST = ("pnorm", "perr", "dnorm", "derr", "objevals")
_L1C_SLOPE0 = dict(logistic=0.5, hinge=1.0, sqhinge=2.0)  # |phi'(0)|


def _l1c_labels(ELL, m, K=None):
    ELL = np.asarray(ELL, dtype=np.float64)
    if ELL.ndim == 1:
        ELL = ELL.reshape(-1, 1)
    if ELL.ndim != 2:
        raise ValueError("Argument ell is neither a vector nor a matrix!")
    if ELL.shape[0] != m:
        raise ValueError("The number of rows in argument D do not match size of ell!")
    if K is not None and ELL.shape[1] not in (1, K):
        raise ValueError(f"ELL has {ELL.shape[1]} columns for {K} fits: one shared label column or one column per fit")
    if not np.all(np.abs(ELL) == 1.0):
        raise ValueError("Argument ell must hold the labels +1 and -1 alone!")
    return np.asfortranarray(ELL)


def _l1c_costs(options, ELL, K):
    """(weights, K x 2 class costs) out of options.weights / options.classcost (None where not given)"""
    w = svm_cost_fields(dict(weights=options.get("weights")), ELL[:, 0])
    weights = None if w is None else w["weights"]
    cc = options.get("classcost")
    if cc is None:
        return weights, None
    cols = [ELL[:, k if ELL.shape[1] > 1 else 0] for k in range(K)]
    if not isinstance(cc, str):
        arr = np.asarray(cc, dtype=np.float64)
        if arr.ndim == 2:
            if arr.shape != (K, 2):
                raise ValueError(f"classcost is not a {K} x 2 array (one (pos, neg) pair per fit)")
            return weights, np.ascontiguousarray([class_cost_pair(arr[k], cols[k]) for k in range(K)])
    return weights, np.ascontiguousarray([class_cost_pair(cc, cols[k]) for k in range(K)])


def l1classifier_lambda_max(D, ell, options=None):
    """The smallest lambda whose l1 classifier is x = 0 when every coefficient is penalised:
    C*|phi'(0)|*max over w_j > 0 of |sum_i c_i*ell_i*D_ij| / w_j, with phi'(0) = -1/2 (logistic), -1 (hinge), -2
    (sqhinge).  With an unpenalised column (w_j = 0) the all-zero model is in general not optimal at this lambda."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    return _classifier_lambda_max(D, ell, options)


def _classifier_lambda_max(D, ell, options, groups=None):
    """l1classifier_lambda_max's body; ``groups`` = (sizes, groupweights): groupclassifier_lambda_max's, the l1 weights
    are not read then"""
    from ._lib import is_sparse
    D = _matrix(D, "D", sparse_ok=is_sparse(D))  # (a sparse D: the one product below is SciPy's)
    ELL = _l1c_labels(ell, D.shape[0], 1)
    loss = options.get("lossfunction", "logistic")
    from .l1class import loss_code
    loss_code(loss)
    weights, cc = _l1c_costs(options, ELL, 1)
    e = ELL[:, 0]
    c = np.ones(e.size) if weights is None else weights.copy()
    if cc is not None:
        c = c * np.where(e > 0, cc[0][0], cc[0][1])
    Cv = is_positive_real(options.get("C", 1.0), "options.C")
    if groups is not None:
        return Cv * _L1C_SLOPE0[loss.lower()] * _group_lambda_max(D, c * e, groups[0], groups[1])
    pw = penalty_fields(dict(l1weights=options.get("l1weights")), D.shape[1])
    g = np.abs(np.asarray(D.T @ (c * e), dtype=np.float64)).reshape(-1)
    if pw is not None:
        live = pw["l1weights"] > 0
        g = g[live] / pw["l1weights"][live]
    return Cv * _L1C_SLOPE0[loss.lower()] * (float(g.max()) if g.size else 0.0)


def l1classifier_multi(D, ELL, lams, options=None):
    """results = l1classifier_multi(D, ELL, lams, options): K sparse linear classifiers over ONE D, dense
    or scipy.sparse (q43), in one run -- a regularisation path, a grid, several label columns or losses:

        minimise C*sum_i c_ik*phi_k(ell_ik*(D*x)_i) + lambda_k*sum_j w_j*|x_j| + ridge_k/2*||x||^2   (x >= 0 where nonnegative_k)

    ``D``: dense or scipy.sparse, any shape (m < n included).  ``ELL``: labels +-1, a vector or m x 1 (shared by all fits) or m x K.
    ``lams``: the K values lambda_k >= 0.  ``options['lossfunction']`` ('logistic' by default, 'hinge', 'sqhinge') is one
    string or K of them; ``ridge`` and ``nonnegative`` are scalars or K values; ``l1weights`` (n values >= 0; 0 leaves a
    coefficient unpenalised -- an intercept is a column of ones with weight 0), ``weights`` (m values >= 0) and ``C``
    (default 1) are shared; ``classcost`` is a pair, 'balanced' or a K x 2 array.  rho, abstol, reltol, maxiters,
    domaxiters, objevals, check_every and nodualerror are the plain loop's; ``z0`` / ``u0`` are (m + n) x K (default
    zeros: the m rows of D above the n coefficients), x0 (n x K) is checked and never read; ``xsolve`` is 'auto',
    'inverse' or 'trsv'.  The loop is admm.m's with A = [D; I], B = -1, c = 0 and stopcond 'standard'.

    Returns xopt (n x K), zopt, uopt ((m + n) x K), steps (K), pnorm / perr (max(steps) x K, NaN past a fit's last
    step), dnorm / derr unless nodualerror = 1, objevals with options['objevals'], objopt, runtime, solverruntime, chunk,
    lams and xsolve.  fast, convtest, relax, adaptive, comm, parallel, a stopcond other than 'standard' and the loss '01'
    are refused by name.

    On a scipy.sparse D every x-update is conjugate gradients on (D'D + I) x = D'(z1 - u1) + (z2 - u2), all fits in
    lock-step over one sparse product: nothing n x n is stored.  ``xsolve`` is 'auto' or 'cg' ('inverse' and 'trsv' are
    refused by name), ``cg_tol`` / ``cg_maxit`` (1e-12 / 200) bound a solve, and the result reads ``xsolve = 'cg'`` and
    adds ``nnz``, ``cg_iters_total`` and ``cg_capped_updates`` (K values each).

    Held-out folds, on a scipy.sparse D: ``options['foldid']`` (m integer fold ids >= 0) together with
    ``options['heldout']`` (K integers: the fold fit k leaves out, -1 for none) give fit k the cost c_ik*[foldid_i !=
    heldout_k]: its minimiser is that of the classifier on the rows it keeps.  The result then carries ``heldout_loss``,
    ``heldout_errors`` and ``heldout_weight`` (K values each) over the rows the fit held out, at D*z2 with z2 the
    coefficient block of zopt: sum c_i*phi(ell_i*t_i) (without C), sum c_i*[ell_i*t_i <= 0] and sum c_i, c_i = weights_i *
    class cost.  One of the two options without the other is refused; ``options['obsweights']`` is refused by name (the
    classifier's option is ``weights``), and on a dense D both options are.  ``l1classifier_cv`` builds a
    cross-validation out of them."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    return _run_multi_classifier(D, ELL, lams, options, "l1classifier_multi", time.perf_counter())


def _run_multi_classifier(D, ELL, lams, options, who, t0, groups=None):
    """the body of l1classifier_multi and of groupclassifier_multi (q48): the refusals, the fits, the owner, one run.
    ``groups``: the sizes of groupclassifier_multi; options.groupweights and options.l1 are read beside them alone, and
    the result carries ``groups``"""
    from ._lib import is_sparse
    from .l1class import L1Classifier, loss_code
    sparse = is_sparse(D)  # the matrix-free object, no limit on n
    if sparse:
        _sparse_refusals(options, who, stopcond=True, folds=True)
    else:
        _dense_multi_refusals(options, who)
    D = _matrix(D, "D", sparse_ok=sparse)
    m, n = D.shape
    lam = _lambda_vector(lams)
    K = int(lam.size)
    ELL = _l1c_labels(ELL, m, K)
    loss = options.get("lossfunction", "logistic")
    losses = [loss] * K if isinstance(loss, str) else list(loss)
    if len(losses) != K:
        raise ValueError("options.lossfunction is neither one string nor a list with one string per fit!")
    for k, v in enumerate(losses):
        loss_code(v, k)
    ridge, nonneg, w, grouped = _fit_penalties(options, n, K, groups)
    Cv = is_positive_real(options.get("C", 1.0), "options.C")
    weights, class_cost = _l1c_costs(options, ELL, K)
    starts = _start_matrices(options, dict(x0=n, z0=m + n, u0=m + n), K, "fit")
    prepare, finish = [_cost_setter(weights, class_cost),
                       None if grouped is None else lambda obj: obj.set_groups(*grouped)], None
    if sparse and (options.get("foldid") is not None or options.get("heldout") is not None):
        if options.get("foldid") is None:
            raise ValueError("options.heldout needs options.foldid: the fold of every observation")
        if options.get("heldout") is None:
            raise ValueError("options.foldid needs options.heldout: the fold every fit leaves out (K values, -1 for none)")
        from .sparse_lasso import observation_arrays
        fold, held = observation_arrays(None, options["foldid"], options["heldout"], m, K)[1:3]
        prepare.append(lambda obj: obj.set_folds(fold, held))

        def finish(obj, res):
            res["heldout_loss"], res["heldout_errors"], res["heldout_weight"] = obj.heldout()
    if sparse:
        from .sparse_l1class import SparseL1Classifier
        obj = SparseL1Classifier(D, ELL, lam, losses, ridge, nonneg, w, C=Cv, xsolve=options.get("xsolve", "auto"),
                                 device=int(options.get("device", 0)))
    else:
        obj = L1Classifier(D, ELL, lam, losses, ridge, nonneg, w, C=Cv, xsolve=options.get("xsolve", "auto"),
                           device=int(options.get("device", 0)))
    res = _run_and_close(obj, prepare, finish, check_every=int(options.get("check_every", 0)),
                         z0=starts.get("z0"), u0=starts.get("u0"), nodualerror=int(bool(options.get("nodualerror", 0))),
                         **_pick(options, _LOOP_KEYS + (_CG_KEYS if sparse else ())))
    res["lams"] = lam.copy()
    if grouped is not None:
        res["groups"] = grouped[0].copy()
    res["solverruntime"] = time.perf_counter() - t0
    return res


def l1classifier(D, ell, lam, options=None):
    """results = l1classifier(D, ell, lam, options): ONE sparse linear classifier, ``l1classifier_multi`` with K = 1 --
    l1-regularised logistic regression by default, the l1-SVM with lossfunction 'hinge' or 'sqhinge'.  ``x0`` has n
    entries, ``z0`` / ``u0`` m + n.  Returns vectors and scalars where l1classifier_multi returns columns."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    return _single_classifier(D, ell, lam, options, "l1classifier_multi")


def _single_classifier(D, ell, lam, options, who, groups=None):
    """l1classifier's body, and groupclassifier's with ``groups``"""
    if not np.isscalar(lam) or not np.isreal(lam):
        raise ValueError("Argument lam is not a nonnegative real number!")
    from ._lib import is_sparse
    D = _matrix(D, "D", sparse_ok=is_sparse(D))
    m, n = D.shape
    loss = options.get("lossfunction", "logistic")
    if not isinstance(loss, str):
        raise ValueError("options.lossfunction is not a string!")
    if groups is not None and np.size(options.get("l1", 0.0)) != 1:
        raise ValueError("options.l1 is not a nonnegative real number!")
    for key, v in _start_columns(options, dict(x0=n, z0=m + n, u0=m + n)).items():
        options[key] = v
    res = _run_multi_classifier(D, _colvec(ell, "ell"), [lam], options, who, time.perf_counter(), groups)
    for key in ("xopt", "zopt", "uopt") + _L1C_HIST:
        if key in res:
            res[key] = np.ascontiguousarray(res[key][:, 0])
    res.update(steps=int(res["steps"][0]), objopt=float(res["objopt"][0]), lam=float(res.pop("lams")[0]))
    for key in ("cg_iters_total", "cg_capped_updates"):  # (a sparse D)
        if key in res:
            res[key] = int(res[key][0])
    return res


def l1classifier_path(D, ell, lams=None, options=None):
    """results = l1classifier_path(D, ell, lams, options): the regularisation path of ``l1classifier``, every lambda
    side by side in one run of ``l1classifier_multi``.  ``lams``: an array, or a count (None: ``options['nlambda']``,
    default 10 = one chunk of the passes over D) for a grid log-spaced from ``l1classifier_lambda_max`` down to
    ``options['lambda_min_ratio']`` (default 1e-2) times it.  lambda_max is the smallest lambda with x = 0 only when
    every coefficient is penalised: with an unpenalised column (l1weights of 0, an intercept) the grid's first point
    may not be the all-zero model.  Returns l1classifier_multi's fields plus ``df``, the nonzeros of each column of the
    coefficient block of zopt."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    return _classifier_path(D, ell, lams, options, "l1classifier_multi")


def _group_l1_refusal(options, who):
    """grouplasso_path's rule: with any l1 != 0 the group lambda_max has no closed form"""
    if np.any(np.asarray(options.get("l1", 0.0), dtype=np.float64) != 0):
        raise ValueError(f"{who}: with options.l1 != 0 lambda_max has no closed form: give lams")


def _classifier_path(D, ell, lams, options, who, groups=None):
    """l1classifier_path's body, and groupclassifier_path's with ``groups`` (the result then adds df_groups)"""
    from ._lib import is_sparse
    D = _matrix(D, "D", sparse_ok=is_sparse(D))
    e = _colvec(ell, "ell")
    gs = None if groups is None else group_sizes(groups, options.get("groupweights"), D.shape[1])
    if gs is not None and (lams is None or np.isscalar(lams)):
        _group_l1_refusal(options, "groupclassifier_path")
    lams = _lambda_grid(options, lams, 10, lambda: _classifier_lambda_max(D, e, options, gs), count_ok=True)
    res = _run_multi_classifier(D, e, lams, options, who, time.perf_counter(), None if gs is None else gs[0])
    Z2 = res["zopt"][D.shape[0]:]
    res["df"] = np.count_nonzero(Z2, axis=0).astype(np.int64)
    if gs is not None:
        res["df_groups"] = _df_groups(Z2, gs[0])
    return res


def _df_groups(Z, sizes):
    """per column of Z the groups with a nonzero block"""
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return np.count_nonzero(np.add.reduceat(Z != 0, first, axis=0), axis=0).astype(np.int64)


def l1classifier_cv(D, ell, lams=None, options=None):
    """results = l1classifier_cv(D, ell, lams, options): F-fold cross-validation of ``l1classifier_path`` on a
    scipy.sparse D, every fold fit and every full-data fit side by side in ONE run of ``l1classifier_multi`` over one
    upload of D.  ``lams = None`` or a count: l1classifier_path's grid (``nlambda``, default 10;
    ``lambda_min_ratio``, default 1e-2) from the full-data ``l1classifier_lambda_max``.  With L lambdas and F =
    ``options['nfolds']`` (default 5, at least 2) the object holds (F + 1)*L fits: fit f*L + l leaves fold f out at
    lambda_l, fits F*L + l see every row.

    ``options['foldid']``: m fold ids in [0, nfolds); absent: ``cv_folds(m, nfolds, options.get('seed', 0))``.  A fold fit
    runs at lambda_l * (training weight of fold f / total weight), the weights being ``options['weights']`` or ones:
    one lambda sequence on the per-observation scale, written for this unnormalised objective;
    ``options['scale_lambda'] = 0`` runs every fold at lambda_l itself.  ``options['measure']`` is 'deviance' (the
    default: held-out loss / held-out weight) or 'class' (held-out weighted errors / held-out weight).  ``lossfunction``
    (one string), ``weights``, ``classcost``, ``C``, ``l1weights``, ``ridge`` and ``nonnegative`` (scalars or L values)
    and the loop / CG options are l1classifier_multi's; ``z0`` / ``u0`` ((m + n) x L) start every fold alike.
    ``classcost = 'balanced'`` is computed ONCE from all rows and used by every fold fit: it is not recomputed from a
    fold's training rows.  ``options['heldout']`` is this function's own to set.

    Returns lams, foldid, measure, ``cv_summary``'s cvm, cvsd, index_min, lam_min, index_1se, lam_1se from the chosen
    sums; xopt (n x L), zopt, uopt ((m + n) x L), df, steps, objopt of the full-data fits; fold_steps, fold_lams,
    heldout_loss, heldout_errors, heldout_weight (F x L); nnz, cg_iters_total and cg_capped_updates over all (F + 1)*L
    fits, chunk, runtime and solverruntime.  A dense D raises ValueError."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    return _classifier_cv(D, ell, lams, options, "l1classifier_cv")


def _classifier_cv(D, ell, lams, options, who, groups=None):
    """l1classifier_cv's body, and groupclassifier_cv's with ``groups``: the same layout and arithmetic with the groups set
    on the one object (the result then adds groups and df_groups)"""
    t0 = time.perf_counter()
    from ._lib import is_sparse
    if not is_sparse(D):
        raise ValueError(f"{who} runs on a scipy.sparse D: the held-out folds live on the sparse object "
                         "(SparseL1Classifier)")
    e = _colvec(ell, "ell")
    m, n = D.shape
    F, foldid, scale = _cv_folds(options, who, m, e, "ell")
    measure = options.pop("measure", "deviance")
    if not (isinstance(measure, str) and measure in ("deviance", "class")):
        raise ValueError("options.measure must be 'deviance' or 'class'")
    loss = options.get("lossfunction", "logistic")
    if not isinstance(loss, str):
        raise ValueError("options.lossfunction is not a string!")
    gs = None if groups is None else group_sizes(groups, options.get("groupweights"), n)
    if gs is not None and (lams is None or np.isscalar(lams)):
        _group_l1_refusal(options, who)
    cost = _pick(options, ("lossfunction", "weights", "classcost", "l1weights", "C"))
    lams = _lambda_grid(options, lams, 10, lambda: _classifier_lambda_max(D, e, cost, gs), count_ok=True)
    lams = _lambda_vector(lams, None)
    ELL = _l1c_labels(e, m, 1)
    wf = svm_cost_fields(dict(weights=options.get("weights")), ELL[:, 0])
    cc = options.get("classcost")
    if cc is not None:  # one pair for every fit, 'balanced' from all rows
        if not isinstance(cc, str) and np.ndim(cc) == 2:
            raise ValueError("classcost is one (pos, neg) pair or 'balanced' in l1classifier_cv")
        options["classcost"] = class_cost_pair(cc, ELL[:, 0])
    fold_lams = _cv_layout(options, lams, foldid, F, scale, np.ones(m) if wf is None else wf["weights"], "weights",
                           ("ridge", "nonnegative") + (() if gs is None else ("l1",)), dict(z0=m + n, u0=m + n, x0=n))
    res = _run_multi_classifier(D, e, np.concatenate([fold_lams.reshape(-1), lams]), options, who, time.perf_counter(),
                                None if gs is None else gs[0])
    out = _cv_results(res, lams, foldid, fold_lams, ("heldout_loss", "heldout_errors", "heldout_weight"),
                      "heldout_loss" if measure == "deviance" else "heldout_errors", m, None if gs is None else gs[0],
                      measure=measure)
    out["solverruntime"] = time.perf_counter() - t0
    return out


def _group_lambda_max(D, s, sizes, gw):
    """the smallest lambda whose group-lasso solution is x = 0: max over omega_g > 0 of ||(D's)_g||_2 / omega_g"""
    g = np.asarray(D.T @ s, dtype=np.float64).reshape(-1)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    norms = np.sqrt(np.add.reduceat(g * g, first))
    live = np.ones(norms.size, dtype=bool) if gw is None else gw > 0
    return float(np.max(norms[live] / (1.0 if gw is None else gw[live]))) if live.any() else 0.0


def grouplasso_multi(D, S, lams, groups, options=None):
    """results = grouplasso_multi(D, S, lams, groups, options): K group-lasso or sparse-group-lasso fits over ONE design
    matrix in one run -- ``lasso_multi``'s object on a scipy.sparse D, ``lasso_multi_dense``'s on a
    dense one (m >= n):

        minimise 1/2*||D*x - s_k||^2 + lambda_k*sum_g omega_g*||x_g||_2 + l1_k*sum_i w_i*|x_i| + ridge_k/2*||x||^2
                                                                                    (x >= 0 where nonnegative_k)

    ``groups``: the sizes of the contiguous groups (integers >= 1 that sum to the columns of D), shared by all fits, as
    ``options['groupweights']`` (omega_g >= 0, default 1) is.  ``options['l1']`` is a scalar or K values (default 0);
    ``ridge``, ``nonnegative`` and ``l1weights`` are lasso_multi's.  S, lams, the starts, the loop options, the refusals
    and the result are those of the underlying caller; the result also carries ``groups`` (the sizes)."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    t0 = time.perf_counter()
    from ._lib import is_sparse
    return _run_multi_lasso(D, S, lams, options, "grouplasso_multi", is_sparse(D), t0, groups=groups)


def grouplasso_path(D, s, groups, lams=None, options=None):
    """results = grouplasso_path(D, s, groups, lams, options): the group lasso's regularisation path, every lambda side by
    side in one run of ``grouplasso_multi``.  ``lams = None`` with l1 = 0: ``options['nlambda']`` values
    (default 10) log-spaced from lambda_max = max over omega_g > 0 of ||(D's)_g||_2 / omega_g -- the smallest lambda
    whose solution is x = 0 -- down to ``options['lambda_min_ratio']`` * lambda_max (default 1e-2).  With any l1 != 0 that
    lambda_max has no closed form: ``lams`` must be given (ValueError).  Returns grouplasso_multi's fields plus ``df``,
    the nonzeros of each zopt column, and ``df_groups``, its groups with a nonzero block."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    from ._lib import is_sparse
    D = _matrix(D, "D", sparse_ok=is_sparse(D))
    s = _colvec(s, "s")
    sizes, gw = group_sizes(groups, options.get("groupweights"), D.shape[1])
    if lams is None:
        _group_l1_refusal(options, "grouplasso_path")
    lams = _lasso_grid(D, s, lams, options, lambda: _group_lambda_max(D, s, sizes, gw))
    res = grouplasso_multi(D, s, lams, sizes, options)
    Z = np.asarray(res["zopt"]).reshape(D.shape[1], -1)
    res["df"] = np.count_nonzero(Z, axis=0).astype(np.int64)
    res["df_groups"] = _df_groups(Z, sizes)
    return res


def groupclassifier_lambda_max(D, ell, groups, options=None):
    """The smallest lambda whose group classifier is x = 0 when every group is penalised and l1 = 0:
    C*|phi'(0)|*max over omega_g > 0 of ||(D'(c o ell))_g||_2 / omega_g, c and phi'(0) as in l1classifier_lambda_max.
    With an unpenalised group (omega_g = 0, an intercept) the all-zero model is in general not optimal at this lambda."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    from ._lib import is_sparse
    n = _matrix(D, "D", sparse_ok=is_sparse(D)).shape[1]
    return _classifier_lambda_max(D, ell, options, group_sizes(groups, options.get("groupweights"), n))


def groupclassifier_multi(D, ELL, lams, groups, options=None):
    """results = groupclassifier_multi(D, ELL, lams, groups, options): K group-lasso or sparse-group-lasso classifiers over
    ONE D, dense or scipy.sparse, in one run -- ``l1classifier_multi``'s objects with groups set:

        minimise C*sum_i c_ik*phi_k(ell_ik*(D*x)_i) + lambda_k*sum_g omega_g*||x_g||_2 + l1_k*sum_j w_j*|x_j|
                 + ridge_k/2*||x||^2                                                (x >= 0 where nonnegative_k)

    ``groups``: the sizes of the contiguous groups (integers >= 1 that sum to the columns of D), shared by all fits, as
    ``options['groupweights']`` (omega_g >= 0, default 1; 0 leaves a group unpenalised -- an intercept is a group of one
    with weight 0) is.  ``lams`` holds the group strengths, ``options['l1']`` (a scalar or K values, default 0) the l1
    strengths.  This is ``grouplasso_multi``'s convention.  Everything else -- ELL, the losses, ridge, nonnegative,
    l1weights, weights, classcost, C, the starts, the loop and CG options, foldid / heldout on a sparse D and their
    refusal on a dense one, the refusals and the result -- is l1classifier_multi's; the result also carries ``groups``."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    return _run_multi_classifier(D, ELL, lams, options, "groupclassifier_multi", time.perf_counter(), groups=groups)


def groupclassifier(D, ell, lam, groups, options=None):
    """results = groupclassifier(D, ell, lam, groups, options): ONE group-lasso classifier, ``groupclassifier_multi`` with
    K = 1 (group-lasso logistic regression by default).  Returns vectors and scalars as ``l1classifier`` does."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    return _single_classifier(D, ell, lam, options, "groupclassifier_multi", groups=groups)


def groupclassifier_path(D, ell, groups, lams=None, options=None):
    """results = groupclassifier_path(D, ell, groups, lams, options): the regularisation path of ``groupclassifier``, every
    lambda side by side in one run.  ``lams``: an array, or a count (None: ``options['nlambda']``, default 10) for a grid
    log-spaced from ``groupclassifier_lambda_max`` down to ``options['lambda_min_ratio']`` (default 1e-2) times it; with
    any l1 != 0 that lambda_max has no closed form and ``lams`` must be an array (ValueError).  Returns
    groupclassifier_multi's fields plus ``df``, the nonzeros of each column of the coefficient block of zopt, and
    ``df_groups``, its groups with a nonzero."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    return _classifier_path(D, ell, lams, options, "groupclassifier_multi", groups=groups)


def groupclassifier_cv(D, ell, groups, lams=None, options=None):
    """results = groupclassifier_cv(D, ell, groups, lams, options): ``l1classifier_cv`` with the group penalty (DESIGN.md
    q48) on a scipy.sparse D: the same (F + 1)*L fits in one object, the same lambda scaling by training weight,
    ``classcost = 'balanced'`` from all rows and ``measure``; ``groups`` / ``options['groupweights']`` are shared by all
    fits and ``options['l1']`` is a scalar or L values (for every fold alike, not scaled).  The automatic grid starts at
    ``groupclassifier_lambda_max`` and needs l1 = 0.  Returns l1classifier_cv's fields plus ``groups`` and
    ``df_groups`` of the full-data fits."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    return _classifier_cv(D, ell, lams, options, "groupclassifier_cv", groups=groups)


def _lad_like(kind, D, s, options):
    options = _options(options, "Argument options is not a struct!")
    t0 = time.perf_counter()
    from ._lib import is_sparse
    if is_sparse(D):
        return _lad_like_sparse(kind, D, s, options, t0)
    D = _matrix(D, "D")
    s = _colvec(s, "s")
    m, n = D.shape
    if s.size != m:
        raise ValueError("The number of rows in argument D do not match size of s!")
    loss = loss_fields({k: options.pop(k, None) for k in LOSS_KEYS}, m, kind)
    if loss is not None and "comm" in options:
        raise ValueError("weights / tau / slopes / epsilon / delta have no row-sharded form: options.comm")
    args = _engine_args(options, dict(D=D, s=s), **(loss or {}))
    if options.get("relax", 1) != 1:  # lad.m:124-126, huberfit.m:156-158
        args["userelax"] = 1
    minx, minz, _ = getproxops(kind, args)
    options.update(A=D, B=-1, c=s, m=m, nA=n, nB=m)  # lad.m:140-145
    options["obj"] = _ENGINE_OBJ  # lad.m:148 norm(z,1) | huberfit.m:180 1/2*sum(huber(z))
    results = admm(minx, minz, options)
    results["solverruntime"] = time.perf_counter() - t0
    return results


_SPARSE_REG_HIST = ("pnorm", "perr", "dnorm", "derr", "objevals")


def _sparse_reg_run(D, S, fl, options, starts, weights, nodualerror):
    """the K runs of robustfit_multi on a scipy.sparse D through one SparseRegMulti: the fields
    robustfit_multi returns, plus xsolve, nnz, cg_iters_total and cg_capped_updates (K values each), and dnorm / derr
    when the dual residual is evaluated"""
    from .sparse_reg import SparseRegMulti
    return _run_and_close(SparseRegMulti(D, S, *_reg_columns(fl), device=int(options.get("device", 0))),
                          _weights_setter(weights), check_every=int(options.get("check_every", 0)),
                          nodualerror=int(bool(nodualerror)), z0=starts.get("z0"), u0=starts.get("u0"),
                          **_pick(options, _LOOP_KEYS + _CG_KEYS))


def _reg_columns(fl):
    """_multi_fits' list as the columns RegMulti / SparseRegMulti take: kinds, a, b, epsilon, delta"""
    return ([0 if f[0] == "lad" else 1 for f in fl],) + tuple([f[i] for f in fl] for i in (1, 2, 3, 4))


def _weights_setter(weights):
    return None if weights is None else lambda obj: obj.set_weights(weights)


def _lad_like_sparse(kind, D, s, options, t0):
    """lad / huberfit on a scipy.sparse D: the K = 1 case of the sparse multi-fit object under the
    reference's default nodualerror = 0, the fit axis dropped from every field; vector histories are not recorded"""
    who = "lad" if kind == "lad" else "huberfit"
    _sparse_refusals(options, who, stopcond=True)
    D = _matrix(D, "D", sparse_ok=True)
    s = _colvec(s, "s")
    m, n = D.shape
    if s.size != m:
        raise ValueError("The number of rows in argument D do not match size of s!")
    loss = loss_fields({k: options.get(k) for k in LOSS_KEYS}, m, kind) or {}
    a, b = loss.get("slopes", (1.0, 1.0))
    fl = [(kind, a, b, loss.get("epsilon", 0.0), loss.get("delta", 1.0))]
    starts = _start_columns(options, dict(x0=n, z0=m, u0=m))  # admm.m:252-254: zeros; x0 is checked and never read
    res = _sparse_reg_run(D, np.asfortranarray(s.reshape(m, 1)), fl, options, starts, loss.get("weights"),
                          options.get("nodualerror", 0))
    _drop_fit_axis(res, _SPARSE_REG_HIST)
    del res["chunk"]
    res["solverruntime"] = time.perf_counter() - t0
    return res


def lad(D, s, options=None):
    """results = lad(D, s, options)   (solvers/lad.m:51-154): minimise ||D*x - s||_1.

    Engine-side extension: minimise sum_i w_i*phi(D*x - s)_i with phi(r) = a*max(r - eps, 0) +
    b*max(-r - eps, 0): ``options['weights']`` (m values w_i >= 0), ``options['slopes']`` = (a, b) or ``options['tau']``
    (the tau-quantile: a = tau, b = 1 - tau) and ``options['epsilon']`` (the dead zone of support vector regression)
    change the z-update alone.

    A ``scipy.sparse`` D runs the K = 1 case of ``robustfit_multi``'s sparse object under the default
    stop rule (``nodualerror = 0``): the same fields with the fit axis dropped, no vector histories, and the same refused
    options."""
    return _lad_like("lad", D, s, options if options is not None else {})


def huberfit(D, s, options=None):
    """results = huberfit(D, s, options)   (solvers/huberfit.m:83-186): 1/2*sum(huber(D*x - s)).

    Engine-side extension: minimise sum_i w_i*(r_i >= 0 ? a : b)*H_delta(r_i), r = D*x - s, with
    H_delta(r) = r^2/2 up to |r| = delta and delta*|r| - delta^2/2 beyond: ``options['weights']``, ``options['slopes']`` =
    (a, b) and ``options['delta']`` change the z-update alone.  A ``scipy.sparse`` D: as for lad()."""
    return _lad_like("huberfit", D, s, options if options is not None else {})


def quantilereg(D, s, tau, options=None):
    """results = quantilereg(D, s, tau, options): quantile regression, minimise sum_i w_i*phi_tau(D*x - s)_i with the
    pinball loss phi_tau(z) = tau*max(z, 0) + (1 - tau)*max(-z, 0) on the residual z = D*x - s -- lad() with
    options['tau'].  Where D spans the constant vector, a fraction tau of the residuals is negative at
    the optimum: #(z < 0) <= tau*m <= #(z <= 0).  ``options['weights']`` as for lad()."""
    if not isinstance(options, dict):
        raise TypeError("Argument options is not a struct!")
    if not np.isscalar(tau) or not np.isreal(tau) or not 0.0 < tau < 1.0:
        raise ValueError("tau must lie strictly inside (0, 1)")
    if options.get("tau") is not None or options.get("slopes") is not None:
        raise ValueError("quantilereg sets the slopes itself: options.tau / options.slopes")
    return lad(D, s, dict(options, tau=float(tau)))


_MULTI_HIST = ("pnorm", "perr", "objevals")
_MULTI_FIT_KEYS = ("kind", "tau", "slopes", "epsilon", "delta")


def _multi_fits(fits, m):
    """``fits`` of robustfit_multi as a list of (kind, a, b, epsilon, delta): a list of dicts, or one dict of columns
    (lists of one length; a scalar or string stands for every fit).  Checked per fit by errorcheck.loss_fields; the
    messages name the fit.  Raises before any device work."""
    if isinstance(fits, dict):
        cols = {k: v for k, v in fits.items() if v is not None}
        sizes = {k: len(v) for k, v in cols.items() if isinstance(v, (list, np.ndarray)) or
                 (isinstance(v, tuple) and k != "slopes")}
        if len(set(sizes.values())) > 1:
            raise ValueError("fits: the columns have mixed lengths (" +
                             ", ".join(f"{k}: {n}" for k, n in sorted(sizes.items())) + ")")
        K = next(iter(sizes.values()), 1)
        fits = [{k: (v[i] if k in sizes else v) for k, v in cols.items()} for i in range(K)]
    if not isinstance(fits, (list, tuple)) or len(fits) < 1 or not all(isinstance(f, dict) for f in fits):
        raise ValueError("fits is neither a non-empty list of dicts nor a dict of columns!")
    out = []
    for k, f in enumerate(fits):
        unknown = sorted(set(f) - set(_MULTI_FIT_KEYS))
        if unknown:
            raise ValueError(f"fit {k}: unknown field {unknown[0]!r} (options['weights'] is shared by all fits)")
        kind = f.get("kind", "lad")
        if kind not in ("lad", "huber", "huberfit"):
            raise ValueError(f"fit {k}: kind is neither 'lad' nor 'huber'")
        kind = "lad" if kind == "lad" else "huberfit"
        try:
            lf = loss_fields({key: f.get(key) for key in LOSS_KEYS if key != "weights"}, m, kind) or {}
        except ValueError as e:
            raise ValueError(f"fit {k}: {e}") from None
        a, b = lf.get("slopes", (1.0, 1.0))
        out.append((kind, a, b, lf.get("epsilon", 0.0), lf.get("delta", 1.0)))
    return out


def robustfit_multi(D, S, fits, options=None):
    """results = robustfit_multi(D, S, fits, options): K fits of the loss family of lad() / huberfit()
    over ONE design matrix in one run: one read of D per iteration for a chunk of fits.

    ``S``: the response, a vector or m x 1 (shared by all fits) or m x K (one column per fit).  ``fits``: a list of K
    dicts with the keys ``kind`` ('lad' | 'huber'), ``tau`` or ``slopes``, ``epsilon`` (lad), ``delta`` (huber) -- or one
    dict of such columns.  ``options['weights']`` (m values >= 0) is shared by all fits.  The options of the plain loop
    apply to every fit (rho, abstol, reltol, maxiters, domaxiters, objevals, check_every; x0 / z0 / u0 as n x K, m x K,
    m x K, default zeros); relax, fast and convtest are refused.  Every fit stops on pnorm < perr: the dual residual is
    not evaluated, so fit k equals ``lad(D, s_k, {..., 'nodualerror': 1})`` / ``huberfit(...)``, not the default call.
    Returns xopt (n x K), zopt, uopt (m x K), steps (K), objopt (K), pnorm / perr / objevals (max(steps) x K, NaN past a
    fit's last step), runtime, solverruntime, chunk (fits per pass over D) and fallback.  For n > 448 the fits run one
    after the other through lad / huberfit with nodualerror = 1 and ``results['fallback']`` is True.

    A ``scipy.sparse`` D stays sparse on the device and runs the matrix-free object: every x-update is
    conjugate gradients on D'D x = D'(s + z - u), all fits in lock-step over one sparse product -- no limit on n, m < n
    and rank-deficient D included (the minimum-norm x-update), no ``fallback``.  ``options['nodualerror']`` (default 1,
    as above) set to 0 evaluates the dual residual as well and returns ``dnorm`` / ``derr``; ``cg_tol`` / ``cg_maxit``
    (1e-12 / 200) bound a solve; x0 is checked and never read.  The results carry ``xsolve = 'cg'``, ``nnz``,
    ``cg_iters_total`` and ``cg_capped_updates`` (K values each).  fast, convtest, relax, adaptive, an xsolve other than
    'auto' / 'cg', comm, parallel and a stopcond other than 'standard' are refused by name."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    t0 = time.perf_counter()
    from ._lib import is_sparse
    sparse = is_sparse(D)  # the matrix-free object, no limit on n
    if sparse:
        _sparse_refusals(options, "robustfit_multi", stopcond=True)
    D = _matrix(D, "D", sparse_ok=sparse)
    m, n = D.shape
    S = _response_matrix(S, m)
    fl = _multi_fits(fits, m)
    K = len(fl)
    S = _response_columns(S, K)
    lw = loss_fields(dict(weights=options.pop("weights", None)), m, "lad")
    weights = None if lw is None else lw["weights"]
    for key in ("fast", "convtest"):
        if options.get(key, 0):
            raise ValueError(f"options.{key} is not available in robustfit_multi: call lad / huberfit per fit")
    if options.get("relax", 1) != 1:
        raise ValueError("options.relax is not available in robustfit_multi: call lad / huberfit per fit")
    if options.get("stopcond", "standard") != "standard":
        raise ValueError("options.stopcond: robustfit_multi stops on the primal residual alone ('standard')")
    starts = _start_matrices(options, dict(x0=n, z0=m, u0=m), K, "fit")
    loop = _pick(options, _LOOP_KEYS)
    if sparse:
        res = _sparse_reg_run(D, S, fl, options, starts, weights, options.get("nodualerror", 1))
        res["solverruntime"] = time.perf_counter() - t0
        return res
    if n > 448:  # the one-pass kernel's limit: per-fit engines, same fields
        per = []
        for k, (kind, a, b, eps, delta) in enumerate(fl):
            o = dict(loop, nodualerror=1, slopes=(a, b), **{key: v[:, k] for key, v in starts.items()})
            if kind == "lad":
                o["epsilon"] = eps
            else:
                o["delta"] = delta
            if weights is not None:
                o["weights"] = weights
            per.append(_lad_like(kind, D, S[:, k if S.shape[1] > 1 else 0], o))
        res = _stack_fits(per, _MULTI_HIST)
        res.update(chunk=1, fallback=True, solverruntime=time.perf_counter() - t0)
        return res
    from .reg_multi import RegMulti
    res = _run_and_close(RegMulti(D, S, *_reg_columns(fl), device=int(options.get("device", 0))),
                         _weights_setter(weights), check_every=int(options.get("check_every", 0)), **starts, **loop)
    res.update(fallback=False, solverruntime=time.perf_counter() - t0)
    return res


def quantilereg_multi(D, s, taus, options=None):
    """results = quantilereg_multi(D, s, taus, options): the quantiles ``taus`` (each strictly inside (0, 1)) of one
    response s in one run over D -- robustfit_multi with the pinball loss of quantilereg() per fit and one shared s.
    Column k of xopt / zopt / uopt belongs to taus[k]; ``results['taus']`` repeats them."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    taus = np.atleast_1d(np.asarray(taus, dtype=np.float64)).reshape(-1)
    if taus.size < 1:
        raise ValueError("taus must hold at least one quantile")
    for k, tau in enumerate(taus):
        if not np.isreal(tau) or not 0.0 < tau < 1.0:
            raise ValueError(f"fit {k}: tau must lie strictly inside (0, 1)")
    if options.get("tau") is not None or options.get("slopes") is not None:
        raise ValueError("quantilereg_multi sets the slopes itself: options.tau / options.slopes")
    res = robustfit_multi(D, _colvec(s, "s"), [dict(kind="lad", tau=float(t)) for t in taus], options)
    res["taus"] = taus
    return res


def _single_column_quirk(D):
    """admm.m:151 takes nA from a matrix A only when it has more than one column, and unwrappedadmm.m:81-86 /
    linearsvm.m:221-227 pass no options.nA: with a single-column D the check of admm.m:188-190 (rows of A' against
    nA = 0) fails -- the reference cannot run these solvers on one feature, and neither does the mirror."""
    if D.shape[1] == 1 and D.shape[0] != 1:
        raise ValueError("Number of rows in At (A transpose) do not match number of columns in A, in constraint Ax + Bz = c")
    if D.shape == (1, 1):
        raise ValueError("Given scalar as matrix A with no number of columns nA specified in options struct; cannot infer nA "
                         "- please specify nA in options!")


def unwrappedadmm(zming, D, options=None):
    """results = unwrappedadmm(zming, D, options)   (solvers/unwrappedadmm.m:1-143)

    Transpose-reduction ADMM: minimise g(z) s.t. D*x = z with x = D^+ (z - u)
    (unwrappedadmm.m:76-78).  Forces maxiters=1000, stopcond='both', nodualerror=1
    (unwrappedadmm.m:90-92).  Deviation q14 (documented): explicit options.x0/z0/u0 win
    over the reference's unconditional ``rand`` so that runs are reproducible.
    """
    options = dict(options or {})
    D = _matrix(D, "D")
    m, n = D.shape
    _single_column_quirk(D)
    if options.get("parallel", "none") in ("xminf", "zming", "both"):
        # unwrappedadmm.m:45-74: the x-update becomes the transpose reduction (W = sum D_i'D_i, d = sum D_i'(z_i-u_i),
        # x = W\d: the engine's cached factor of D'D does exactly that) and admm slices the z-prox ('zming').
        options["slices"] = slicemaker(options.get("slices", 0), int(options.get("workers", 1)), m)
        options["parallel"] = "zming" if options["parallel"] == "both" else "none"
    from .api import ProxOp
    if isinstance(zming, ProxOp):
        prob = zming.problem
    elif callable(zming):
        # the reference's own use of this solver: the CALLER's z-prox handle (unwrappedadmm.m:1).  The x-update
        # x = D^+ (z - u) is the linear-SVM engine's (same closure: getProxOps.m:1062-1068 == unwrappedadmm.m:78);
        # the handle runs on device tensors between the two halves of the fused kernel.
        args = _engine_args(options, dict(D=D, Dt=None, ell=np.ones(m), C=1.0, lossfunction="hinge"))
        prob = getproxops("LinearSVM", args)[0].problem
    else:
        raise TypeError("Given zming is not a function handle!")
    xminf = ProxOp(prob, "x")
    options.update(A=D, At=D.T, B=-1, nB=m, c=0, m=m)
    rng = np.random.default_rng()
    for key, size in (("x0", n), ("z0", m), ("u0", m)):  # unwrappedadmm.m:87-89
        if key not in options:
            options[key] = rng.random(size)
    options["maxiters"] = 1000
    options["stopcond"] = "both"
    options["nodualerror"] = 1
    return admm(xminf, zming, options)


def linearsvm(D, ell, C, options=None):
    """results = linearsvm(D, ell, C, options)   (solvers/linearsvm.m:92-246).

    ``options['lossfunction']``: 'hinge' (default), '01', 'logistic' -- C*sum(log(1 + exp(-ell.*(D*x)))) -- or 'sqhinge'
    -- C*sum(max(1 - ell.*(D*x), 0).^2), the L2-loss SVM --, two losses the reference does not have (DESIGN.md q29,
    q34); any other string is the reference's hinge prox with the 0-1 objective.

    Engine-side extension: ``options['weights']`` (m values w_i >= 0) and ``options['classcost']`` (a
    pair (pos, neg), or 'balanced' = (m/(2*m_pos), m/(2*m_neg))) put the cost c_i = w_i*(ell_i > 0 ? pos : neg) on
    observation i: C*sum_i c_i*phi(ell_i*(D*x)_i).  They change the z-update and the objective alone.

    A ``scipy.sparse`` D runs the K = 1 case of ``linearsvm_ovr``'s sparse object: the same fields with
    the class axis dropped, no vector histories, and the same refused options."""
    options = _options(options, "Given options is not a struct! At least pass empty struct!")
    t0 = time.perf_counter()
    if not np.isscalar(C) or np.real(C) < 0:  # linearsvm.m:270-274
        raise ValueError("Given regularization parameter C is not a nonnegative number!")
    C = float(np.real(C))
    ell = _colvec(ell, "ell")
    D = _matrix(D, "D", sparse_ok=True)
    if D.shape[0] != ell.size:
        raise ValueError("Product ell*D is not possible; sizes incompatible!")
    _single_column_quirk(D)
    from ._lib import is_sparse
    if is_sparse(D):
        return _linearsvm_sparse(D, ell, C, options, t0)
    loss = options.get("lossfunction", "hinge")  # linearsvm.m:154-158
    cost = svm_cost_fields({k: options.pop(k, None) for k in SVM_COST_KEYS}, ell)
    if cost is not None and "comm" in options:
        raise ValueError("weights / classcost have no row-sharded form: options.comm")
    args = _engine_args(options, dict(D=D, Dt=None, ell=ell, C=C, lossfunction=loss), **(cost or {}))
    if options.get("parallel", "none") in ("both", "zming", "xminf"):  # linearsvm.m:170-205
        options["parallel"] = "both"
        args["slices"] = options["slices"] = slicemaker(options.get("slices", 0), int(options.get("workers", 1)),
                                                         D.shape[0])
    _, minz, _ = getproxops("LinearSVM", args)
    options["obj"] = _ENGINE_OBJ  # linearsvm.m:231-237
    results = unwrappedadmm(minz, D, options)
    results["solverruntime"] = time.perf_counter() - t0
    return results


def _linearsvm_sparse(D, ell, C, options, t0):
    """linearsvm on a scipy.sparse D: the K = 1 case of the sparse one-vs-rest object, the class axis
    dropped from every field; vector histories are not recorded"""
    _sparse_refusals(options, "linearsvm", also=("Dplus",))
    m, n = D.shape
    loss = options.get("lossfunction", "hinge")
    if not isinstance(loss, str):
        raise ValueError("options.lossfunction is not a string!")
    cost = svm_cost_fields({k: options.get(k) for k in SVM_COST_KEYS}, ell)
    starts = _start_columns(options, dict(x0=n, z0=m, u0=m), np.random.default_rng().random)  # unwrappedadmm.m:87-89
    weights = class_cost = None
    if cost is not None:
        weights = cost.get("weights")
        class_cost = np.array([cost.get("classcost", (1.0, 1.0))], dtype=np.float64)
    res = _sparse_svm_run(D, np.asfortranarray(ell.reshape(m, 1)), C, [loss], options, starts, weights, class_cost)
    _drop_fit_axis(res, _OVR_HIST)
    res["solverruntime"] = time.perf_counter() - t0
    return res


def ovr_label_matrix(labels, classes):
    """ELL (m x K): ell_c = +1 where labels == classes[c], else -1 (examples/mnistsvm.m:136-142)."""
    labels = np.asarray(labels).reshape(-1)
    return np.asfortranarray(np.where(labels[:, None] == np.asarray(classes)[None, :], 1.0, -1.0))


def _ovr_costs(options, ELL):
    """(weights, K x 2 class costs) of linearsvm_ovr out of options.weights / options.classcost (None where not given)"""
    m, K = ELL.shape
    w = svm_cost_fields(dict(weights=options.get("weights")), ELL[:, 0])
    weights = None if w is None else w["weights"]
    cc = options.get("classcost")
    if cc is None:
        return weights, None
    if not isinstance(cc, str):
        try:
            arr = np.asarray(cc, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("classcost is neither a pair (pos, neg), 'balanced' nor a K x 2 array") from None
        if arr.ndim == 2 and arr.shape == (K, 2):
            return weights, np.ascontiguousarray([class_cost_pair(arr[c], ELL[:, c]) for c in range(K)])
        if arr.ndim == 2:
            raise ValueError(f"classcost is not a {K} x 2 array (one (pos, neg) pair per class)")
    return weights, np.ascontiguousarray([class_cost_pair(cc, ELL[:, c]) for c in range(K)])


_OVR_HIST = ("pnorm", "perr", "Hnormsq", "objevals")


def _ovr_loop(options):
    """the loop options of the one-vs-rest pair; maxiters is unwrappedadmm's 1000"""
    loop = _pick(options, ("rho", "abstol", "reltol", "domaxiters", "objevals"))
    if "Hreltol" in options or "Hnormtol" in options:  # admm.m:927-928 (q2): either spelling
        loop["Hnormtol"] = options.get("Hreltol", options.get("Hnormtol"))
    return loop


def _cost_setter(weights, class_cost):
    return None if weights is None and class_cost is None else lambda obj: obj.set_cost(weights, class_cost)


def _sparse_svm_run(D, ELL, C, losses, options, starts, weights, class_cost):
    """the K runs of linearsvm_ovr on a scipy.sparse D through one SparseSvmOvr: the fields
    linearsvm_ovr returns, plus xsolve, nnz, cg_iters_total and cg_capped_updates (K values each)"""
    from .sparse_svm import SparseSvmOvr
    return _run_and_close(SparseSvmOvr(D, ELL, C, losses, device=int(options.get("device", 0))),
                          _cost_setter(weights, class_cost), check_every=int(options.get("check_every", 0)),
                          z0=starts["z0"], u0=starts["u0"], **_ovr_loop(options), **_pick(options, _CG_KEYS))


def linearsvm_ovr(D, labels, C, options=None):
    """results = linearsvm_ovr(D, labels, C, options): one linearsvm (solvers/linearsvm.m:92-246) per class of
    ``labels`` against the rest, as examples/mnistsvm.m:88-102 trains them, in ONE run over D.

    ``labels``: length-m vector of class ids.  ``options['classes']`` (default: the sorted unique labels) selects and
    orders the K columns and may name a class more than once; ``options['lossfunction']`` is one string or a list with
    one entry per column ('hinge', '01', 'logistic', 'sqhinge', mixed freely; see ``linearsvm``).  ``options['weights']``
    (m values >= 0) is shared by all classes; ``options['classcost']`` is one pair (pos, neg) for every class,
    'balanced' (per class, from that class's counts) or a K x 2 array.  ``x0`` / ``z0`` / ``u0`` are
    n x K / m x K matrices (missing: random, unwrappedadmm.m:87-89).
    The options of the plain loop apply to every class (rho, abstol, reltol, Hnormtol, domaxiters, objevals,
    check_every); maxiters is 1000, stopcond 'both', nodualerror 1 (unwrappedadmm.m:90-92).
    Returns classes, xopt (n x K), zopt, uopt (m x K), steps (K), pnorm / perr / Hnormsq / objevals (max(steps) x K,
    NaN past a class's last step), objopt (K), runtime, solverruntime.  Vector histories are not recorded.
    For n > 448 the classes run one after the other through ``linearsvm`` and the same fields come back.

    ``D`` may be any ``scipy.sparse`` matrix or array: it is converted to canonical CSC and stays sparse
    on the device, and the x-update D^+(z - u) is conjugate gradients on D'D x = D'(z - u) for all classes in lock-step
    (``cg_tol``, ``cg_maxit`` as for ``xsolve = 'cg'``; x0 is never read: the first solve starts from 0).  There is no
    limit on n; the results also carry ``xsolve`` = 'cg', ``nnz``, ``cg_iters_total`` and ``cg_capped_updates`` (K values
    each).  ``fast``, ``convtest``, ``relax`` != 1, ``adaptive``, ``xsolve`` other than auto / cg, ``Dplus``, ``comm`` and
    ``parallel`` raise ValueError.
    """
    options = _options(options, "Given options is not a struct! At least pass empty struct!", optional=True)
    t0 = time.perf_counter()
    if not np.isscalar(C) or np.real(C) < 0:  # linearsvm.m:270-274
        raise ValueError("Given regularization parameter C is not a nonnegative number!")
    C = float(np.real(C))
    labels = _colvec(labels, "labels")
    D = _matrix(D, "D", sparse_ok=True)
    from ._lib import is_sparse
    sparse = is_sparse(D)  # the matrix-free object, no limit on n
    m, n = D.shape
    if labels.size != m:
        raise ValueError("Product ell*D is not possible; sizes incompatible!")  # linearsvm.m:283-286
    _single_column_quirk(D)
    if sparse:
        _sparse_refusals(options, "linearsvm_ovr", also=("Dplus",))
    classes = np.asarray(options["classes"] if "classes" in options else np.unique(labels), dtype=np.float64)
    if classes.ndim != 1 or classes.size < 1:
        raise ValueError("options.classes is not a non-empty vector of class ids!")
    K = int(classes.size)
    loss = options.get("lossfunction", "hinge")  # linearsvm.m:154-158
    losses = [loss] * K if isinstance(loss, str) else list(loss)
    if len(losses) != K or not all(isinstance(v, str) for v in losses):
        raise ValueError("options.lossfunction is neither one string nor a list with one string per class!")
    starts = _start_matrices(options, dict(x0=n, z0=m, u0=m), K, "class",  # unwrappedadmm.m:87-89, per class
                             np.random.default_rng().random)
    for key in ("fast", "convtest"):
        if options.get(key, 0):
            raise ValueError(f"options.{key} is not available in linearsvm_ovr: call linearsvm per class")
    if options.get("relax", 1) != 1:
        raise ValueError("options.relax is not available in linearsvm_ovr: call linearsvm per class")
    ELL = ovr_label_matrix(labels, classes)
    weights, class_cost = _ovr_costs(options, ELL)
    loop = _ovr_loop(options)
    res = dict(classes=classes)
    if sparse:
        res.update(_sparse_svm_run(D, ELL, C, losses, options, starts, weights, class_cost))
        res["solverruntime"] = time.perf_counter() - t0
        return res
    if n > 448:  # the one-pass kernel's limit: per-class engines, same fields
        per = []
        for c in range(K):
            o = dict(loop, lossfunction=losses[c], x0=starts["x0"][:, c], z0=starts["z0"][:, c], u0=starts["u0"][:, c],
                     record_history=0)
            if weights is not None:
                o["weights"] = weights
            if class_cost is not None:
                o["classcost"] = tuple(class_cost[c])
            per.append(linearsvm(D, ELL[:, c], C, o))
        res.update(_stack_fits(per, _OVR_HIST), solverruntime=time.perf_counter() - t0)
        return res
    from .engine import SvmOvr
    res.update(_run_and_close(SvmOvr(D, ELL, C, losses, Dplus=options.get("Dplus"), device=int(options.get("device", 0))),
                              _cost_setter(weights, class_cost), check_every=int(options.get("check_every", 0)),
                              **starts, **loop))
    res["solverruntime"] = time.perf_counter() - t0
    return res


def quadraticprogram(P, q, r, cons1, cons2, options=None):
    """results = quadraticprogram(P, q, r, cons1, cons2, options)  (solvers/quadraticprogram.m:99-246)

    'bounded' form: cons1 = lb, cons2 = ub vectors.  'standard' form: one matrix D and one vector s
    (either order, quadraticprogram.m:321-329) for D*x = s, x >= 0.  ``options['altproxg']`` (a handle on
    device tensors) replaces the z-prox as in quadraticprogram.m:221-227.
    """
    options = _options(options, "Argument options is not a struct!")
    t0 = time.perf_counter()
    P = _matrix(P, "P")
    if P.shape[0] != P.shape[1]:
        raise ValueError("Argument P is not a square matrix!")
    q = _colvec(q, "q")
    if q.size != P.shape[0]:
        raise ValueError("The dimensions of square matrix P and vector q do not match!")
    c1, c2 = np.asarray(cons1, dtype=np.float64), np.asarray(cons2, dtype=np.float64)
    vec1, vec2 = (c1.ndim <= 1 or 1 in c1.shape), (c2.ndim <= 1 or 1 in c2.shape)
    if not vec1 and not vec2:
        raise ValueError("It appears that both constraint inputs are matrices! If trying to use standard "
                         "constraint form, only one can be a matrix.")  # quadraticprogram.m:361-363
    if not (vec1 and vec2):  # 'standard': D*x = s, x >= 0   (quadraticprogram.m:319-345)
        Dm, sv = (c2, c1) if vec1 else (c1, c2)
        sv = sv.reshape(-1)
        if Dm.shape[1] != P.shape[0]:
            raise ValueError("Number of columns in constraint matrix in standard form do not match lengths of "
                             "P and q!")  # quadraticprogram.m:348-349
        if Dm.shape[0] != sv.size:
            raise ValueError("Number of rows in constraint matrix in standard form does not match length of "
                             "constraint vector! (D and s in standard form)")  # quadraticprogram.m:351-353
        n = P.shape[0]
        rho = float(options.get("rho", 1.0))
        args = _engine_args(options, dict(P=P, q=q, D=Dm, s=sv, rho=rho, n=n, constraint="standard", r=float(r)))
        minx, minz, _ = getproxops("quadraticprogram", args)
        if callable(options.get("altproxg")):
            minz = options["altproxg"]
        options.update(A=1, B=-1, c=0, m=n, nA=n, nB=n)
        options["obj"] = _ENGINE_OBJ  # quadraticprogram.m:242
        results = admm(minx, minz, options)
        results["solverruntime"] = time.perf_counter() - t0
        return results
    lb, ub = c1.reshape(-1), c2.reshape(-1)
    if lb.size != ub.size:
        raise ValueError("Lengths of lower and upper bound constraints on solution x do not match!")
    if lb.size != P.shape[0]:
        raise ValueError("Bound vectors do not match predicted length of solution x!")
    if np.array_equal(np.maximum(lb, ub), lb):  # quadraticprogram.m:319-322 swap
        lb, ub = ub, lb
    elif not np.array_equal(np.maximum(lb, ub), ub):
        raise ValueError("Given constraint variables do not specify an upper and lower bound on solution x!")
    n = P.shape[0]
    rho = float(options.get("rho", 1.0))
    args = _engine_args(options, dict(P=P, q=q, lb=lb, ub=ub, rho=rho, n=n, constraint="bounded", r=float(r)))
    minx, minz, _ = getproxops("quadraticprogram", args)
    if callable(options.get("altproxg")):  # quadraticprogram.m:221-227
        minz = options["altproxg"]
    options.update(A=1, B=-1, c=0, m=n, nA=n, nB=n)
    options["obj"] = _ENGINE_OBJ  # quadraticprogram.m:242
    results = admm(minx, minz, options)
    results["solverruntime"] = time.perf_counter() - t0
    return results


def linearprogram(b, D, s, options=None):
    """results = linearprogram(b, D, s, options)   (solvers/linearprogram.m:81-185)

    minimise b'*x subject to D*x = s, x >= 0.  The reference solves the (n+m) x (n+m) KKT system in
    every x-update (getProxOps.m:1363); here it is reduced once on the host to x = K*y + k0 and the
    per-iteration n x n GEMV, the pos() prox, the u-update and the residuals run on the device.
    """
    options = _options(options, "Given options is not a struct! At least pass empty struct!", optional=True)
    t0 = time.perf_counter()
    D = _matrix(D, "D")
    b = _colvec(b, "b")
    s = _colvec(s, "s")
    m, n = D.shape
    if b.size != n:
        raise ValueError("Number of columns in D do not match length of vector b!")  # linearprogram.m:241-244
    if s.size != m:
        raise ValueError("Number of rows in D does not match length of vector s!")
    rho = is_positive_real(options["rho"], "options.rho") if "rho" in options else 1.0
    args = _engine_args(options, dict(D=D, Dt=D.T, b=b, s=s, n=n, rho=rho))
    minx, minz, _ = getproxops("LinearProgram", args)
    if callable(options.get("altproxg")):  # linearprogram.m:158-164
        minz = options["altproxg"]
    options.update(A=1, B=-1, c=0, m=n, nA=n, nB=n)  # linearprogram.m:172-177
    options["obj"] = _ENGINE_OBJ  # linearprogram.m:178  b'*x
    results = admm(minx, minz, options)
    results["solverruntime"] = time.perf_counter() - t0
    return results


def basispursuit(D, s, options=None):
    """results = basispursuit(D, s, options)   (solvers/basispursuit.m:52-145).

    The projector P = I - D'(DD')^-1 D and q = D'(DD')^-1 s (basispursuit.m:116-120) are formed once by the
    engine on the device (MFMA GEMMs + Cholesky + explicit m x m inverse); the per-iteration n x n GEMV and the
    shrinkage run on the device.
    """
    options = _options(options, "Given options is not a struct! At least pass empty struct!")
    t0 = time.perf_counter()
    D = _matrix(D, "D")
    s = _colvec(s, "s")
    mD, nD = D.shape
    if mD == nD and mD == s.size:
        raise ValueError("Square matrix problem Dx = s; don't need Basis Pursuit to solve this!")
    if mD > nD and mD == s.size:
        raise ValueError("Overdetermined system Dx = s; use Unwrapped ADMM solver instead.")
    if mD != s.size:
        raise ValueError("The number of rows in matrix D must match the number of rows in signal vector s!")
    n = nD
    minx, minz, _ = getproxops("BasisPursuit", _engine_args(options, dict(D=D, s=s)))
    options.update(A=1, B=-1, c=0, m=n, nA=n, nB=n)
    options["obj"] = _ENGINE_OBJ  # basispursuit.m:140 norm(x,1)
    results = admm(minx, minz, options)
    results["solverruntime"] = time.perf_counter() - t0
    return results


def totalvariation(s, lam, options=None):
    """results = totalvariation(s, lambda, options)   (solvers/totalvariation.m:62-167)

    minimise 1/2*||x - s||_2^2 + lambda*sum|x_{i+1} - x_i| (1-D signal).  The difference operator
    D = spdiags([1 -1], 0:1, n, n) (totalvariation.m:127) is never formed on the device: its
    stencils are fused into the kernels and (I + rho*D'D) is solved by parallel recurrences.
    """
    import scipy.sparse as sp

    options = _options(options, "Given options is not a struct! At least pass empty struct!")
    t0 = time.perf_counter()
    if not np.isscalar(lam) or np.real(lam) < 0:  # totalvariation.m:190-194
        raise ValueError("Given lambda parameter is not a nonnegative number!")
    lam = float(np.real(lam))
    s = _colvec(s, "s")
    n = s.size
    if n == 1:  # admm.m:145-148: totalvariation.m:151 hands admm a 1 x 1 matrix D and no options.nA
        raise ValueError("Given scalar as matrix A with no number of columns nA specified in options struct; cannot infer nA "
                         "- please specify nA in options!")
    args = _engine_args(options, dict(s=s))
    args["lambda"] = lam
    xmin, zmin, _ = getproxops("TotalVariation", args)
    D = sp.diags([np.ones(n), -np.ones(n - 1)], [0, 1], shape=(n, n), format="csr") if n <= (1 << 22) else \
        _ShapeOnly((n, n))
    options.update(A=D, At=None, B=-1, mB=n, nB=n, c=0, m=n)  # totalvariation.m:151-157
    options["obj"] = _ENGINE_OBJ  # totalvariation.m:134-135
    results = admm(xmin, zmin, options)
    results["solverruntime"] = time.perf_counter() - t0
    return results


def totalvariation2d(S, lam, options=None):
    """results = totalvariation2d(S, lambda, options) -- engine-side extension (the reference's
    totalvariation.m is 1-D): TV denoising of an image, anisotropic by default,

        minimise 1/2*||X - S||_F^2 + lambda*(sum|X[i+1,j] - X[i,j]| + sum|X[i,j+1] - X[i,j]|),

    or with ``options['isotropic'] = 1`` the isotropic (Rudin-Osher-Fatemi) norm, which does not favour axis-aligned edges,

        minimise 1/2*||X - S||_F^2 + lambda*sum_ij sqrt((X[i+1,j] - X[i,j])^2 + (X[i,j+1] - X[i,j])^2)

    (a difference that leaves the image counts as 0) -- as ADMM on D*x - z = 0 with D = [Dv; Dh] (2N x N forward
    differences, x = X(:) column-major).  The isotropic z-update shrinks each pixel's pair of differences as a block;
    everything else is shared.  The
    x-update (I + rho*D'D) x = s + rho*D'(z - u) is solved spectrally where the height has a column transform (8 to
    4096 rows, or a power of two up to 8192): column DCT, a row stage (Toeplitz kernel, row DCT or exact tridiagonal
    solve, whichever applies to this width and rho), inverse column DCT -- and matrix-free by warm-started CG otherwise
    or with ``options['xsolve'] = 'cg'`` (``options['cg_tol']``, default 1e-11 relative; ``results['cg_capped_updates']``
    counts x-updates that ended on the step cap); nothing is factored.  ``results['tv2d_row_stage']`` names the row
    stage the run took: 'green', 'coop', 'dct', 'thomas', or 'cg' without a spectral x-update.  ``xopt`` is returned as
    an image.
    """
    options = _options(options, "Given options is not a struct! At least pass empty struct!", optional=True)
    t0 = time.perf_counter()
    if not np.isscalar(lam) or np.real(lam) < 0:
        raise ValueError("Given lambda parameter is not a nonnegative number!")
    img = np.asarray(S, dtype=np.float64)
    if img.ndim != 2:
        raise ValueError("Argument S is not an image (2-D array)!")
    H, W = img.shape
    N = H * W
    args = _engine_args(options, dict(s=img))
    args["lambda"] = float(np.real(lam))
    if "isotropic" in options:
        args["isotropic"] = options.pop("isotropic")
    xmin, zmin, _ = getproxops("TotalVariation2D", args)
    options.update(A=_ShapeOnly((2 * N, N)), At=None, B=-1, nA=N, nB=2 * N, c=0, m=2 * N)
    options["obj"] = _ENGINE_OBJ
    results = admm(xmin, zmin, options)
    results["xopt"] = results["xopt"].reshape((H, W), order="F")
    results["solverruntime"] = time.perf_counter() - t0
    return results


class _ShapeOnly:
    """Stand-in for options.A when materialising the sparse operator would only cost memory."""

    def __init__(self, shape):
        self.shape = shape


def model(P, Q, r, s, options=None):
    """results = model(P, Q, r, s, options)   (solvers/model.m:47-143)

    minimise 1/2*||P*x - r||_2^2 + 1/2*||Q*z - s||_2^2 subject to x - z = 0.  The host forms the
    Gram data exactly as model.m:111-121 does and passes it to ``getproxops('model', args)``; the
    matrices themselves travel along (engine-side extension) so that the device can evaluate the
    objective of model.m:133-134 when ``objevals`` is set.
    """
    options = _options(options, "Given options is not a struct! At least pass empty struct!", optional=True)
    t0 = time.perf_counter()
    P = _matrix(P, "P")
    Q = _matrix(Q, "Q")
    r = _colvec(r, "r")
    s = _colvec(s, "s")
    if P.shape[0] != Q.shape[0]:  # model.m:204-211
        raise ValueError("Number of rows in P do not match number of rows in Q!")
    if P.shape[1] != Q.shape[1]:
        raise ValueError("Number of columns in P do not match number of columns in Q!")
    if P.shape[0] != r.size:
        raise ValueError("Number of rows in P does not match length of vector r!")
    if Q.shape[0] != s.size:
        raise ValueError("Number of rows in Q does not match length of vector s!")
    n = P.shape[1]
    rho = is_positive_real(options["rho"], "options.rho") if "rho" in options else 1.0
    args = dict(PtP=P.T @ P, Ptr=P.T @ r, QtQ=Q.T @ Q, Qts=Q.T @ s, n=n, rho=rho, P=P, Q=Q, r=r, s=s)
    minx, minz, _ = getproxops("Model", _engine_args(options, args))
    options.update(A=1, B=-1, c=0, m=n, nA=n, nB=n)  # model.m:124-130
    options["obj"] = _ENGINE_OBJ
    results = admm(minx, minz, options)
    results["solverruntime"] = time.perf_counter() - t0
    return results


def covarianceselection(D, lam, options=None):
    """results = covarianceselection(D, lambda, options)   (solvers/covarianceselection.m:140-173).

    Sparse inverse covariance selection: minimise trace(S*X) - log det X + lambda*||X||_1 over X with S = cov(D)
    (D: m samples x n variables).  S is formed on the device (columns centred, then the MFMA Gram / (m - 1)); the loop
    runs on the n^2 entries of X, Z, U with A = 1, B = -1, c = 0 and the eigen-step x-update of getProxOps.m:1487-1495.
    xopt, zopt, uopt (and x0, z0, u0) come back as n x n matrices; histories keep their n^2-row shape.
    """
    options = _options(options, "Given options is not a struct! At least pass empty struct!", optional=True)
    t0 = time.perf_counter()
    D = _matrix(D, "D")
    lam = is_positive_real(lam, "lambda")
    n = D.shape[1]
    args = _engine_args(options, dict(D=D))
    args["lambda"] = lam
    minx, minz, _ = getproxops("CovarianceSelection", args)
    options.update(A=1, B=-1, c=0, m=n, nA=n, nB=n)  # covarianceselection.m:157-163 (x0 = z0 = u0 = zeros(n, n))
    options["obj"] = _ENGINE_OBJ  # covarianceselection.m:169  trace(S*x) - log(det(x)) + lambda*norm(z(:), 1)
    results = admm(minx, minz, options)
    for key in ("xopt", "zopt", "uopt", "x0", "z0", "u0"):
        if key in results:
            results[key] = np.asarray(results[key]).reshape((n, n), order="F")
    results["solverruntime"] = time.perf_counter() - t0
    return results


# ---- covariance selection, K fits over one S
_COVSEL_HIST = ("pnorm", "perr", "dnorm", "derr", "objevals")


def _covsel_S(D, options):
    """(D, S): the samples as a matrix, or options['S'] (popped) in their place -- exactly one of the two"""
    S = options.pop("S", None)
    if (D is None) == (S is None):
        raise ValueError("covariance selection takes either the samples D or options.S, not both and not neither")
    if S is None:
        D = _matrix(D, "D")
        if D.shape[0] < 2:
            raise ValueError("cov(D) needs at least two samples (rows of D)")
        return D, None
    S = _matrix(S, "S")
    if S.shape[0] != S.shape[1]:
        raise ValueError("options.S is not a square matrix!")
    return None, S


def _host_cov(D, S):
    if S is not None:
        return S
    C = np.atleast_2d(np.cov(D, rowvar=False))
    return 0.5 * (C + C.T)


def covarianceselection_lambda_max(D, options=None):
    """lambda_max = max over i != j of |S_ij| with S = cov(D) (or ``options['S']`` in place of D): at and above it the
    covariance-selection fit is diagonal.  0 for n = 1."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    S = _host_cov(*_covsel_S(D, options))
    off = np.abs(S - np.diag(np.diag(S)))
    return float(off.max()) if off.size else 0.0


def _covsel_multi_refusals(options):
    for key in ("fast", "convtest", "adaptive"):
        if options.get(key, 0):
            raise ValueError(f"options.{key} is not available in covarianceselection_multi: call covarianceselection "
                             "per fit")
    if options.get("relax", 1) != 1:
        raise ValueError("options.relax is not available in covarianceselection_multi: call covarianceselection per fit")
    for key in ("comm",):
        if options.get(key) is not None:
            raise ValueError(f"options.{key} is not available in covarianceselection_multi")
    if options.get("parallel", "none") not in ("none", 0, None):
        raise ValueError("options.parallel is not available in covarianceselection_multi")
    if options.get("stopcond", "standard") != "standard":
        raise ValueError("options.stopcond: covarianceselection_multi runs the 'standard' stop rule alone")


def covarianceselection_multi(D, lams, options=None):
    """results = covarianceselection_multi(D, lams, options): K covariance-selection fits (``covarianceselection``) over
    one S = cov(D) in ONE run -- a regularisation path or a cross-validation grid of

        minimise trace(S*X) - log det X + lambda_k*||X||_1

    ``lams``: the K values lambda_k > 0.  ``options['rho']`` is a scalar or K values (the eigen-step caches no factor, so
    every fit may have its own); ``options['S']`` (n x n, symmetric) replaces D (pass ``D = None``).  ``z0`` / ``u0`` are
    n x n x K (default zeros); ``nodualerror`` (default 0: both residuals) set to 1 stops on the primal residual alone;
    abstol, reltol, maxiters, domaxiters, objevals and check_every apply to every fit.  For n <= 96 every fit runs in a
    workgroup of its own, the whole iteration in one kernel; for n > 96 the fits run one after the other through
    ``covarianceselection`` and the same fields come back.

    Returns xopt, zopt, uopt (n x n x K), steps (K), pnorm / perr (max(steps) x K, NaN past a fit's last step), dnorm /
    derr unless nodualerror = 1, objevals with options['objevals'], objopt (K), runtime, solverruntime, lams, rhos and
    jacobi_sweeps (K).  fast, convtest, relax, adaptive, comm, parallel and a stopcond other than 'standard' are refused
    by name."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    t0 = time.perf_counter()
    _covsel_multi_refusals(options)
    D, S = _covsel_S(D, options)
    n = int((D if S is None else S).shape[1])
    lam = _lambda_vector(lams, zero_ok=False)
    K = int(lam.size)
    rhos = np.asarray(_per_fit(options.get("rho", 1.0), K, "rho", lambda v: is_positive_real(v, "options.rho")),
                      dtype=np.float64)
    if not np.all(np.isfinite(rhos)):
        raise ValueError("options.rho is not finite")
    starts = {}
    for key in ("z0", "u0"):
        if options.get(key) is not None:
            v = np.asarray(options[key], dtype=np.float64)
            if v.shape != (n, n, K):
                raise ValueError(f"options.{key} is not an {n} x {n} x {K} array (one n x n start per fit)!")
            starts[key] = v
    nodual = int(bool(options.get("nodualerror", 0)))
    loop = _pick(options, ("abstol", "reltol", "maxiters", "domaxiters", "objevals"))
    from ._lib import COVSEL_SMALL_MAX
    if n > COVSEL_SMALL_MAX:  # a fit no longer fits one workgroup's LDS: per-fit engines, same fields
        per = []
        for k in range(K):
            o = dict(loop, rho=float(rhos[k]), nodualerror=nodual, record_history=0,
                     **{key: v[:, :, k] for key, v in starts.items()})
            if "device" in options:
                o["device"] = options["device"]
            if "check_every" in options:
                o["check_every"] = options["check_every"]
            per.append(covarianceselection(D, float(lam[k]), o) if S is None else _covsel_single_S(S, float(lam[k]), o))
        hist = tuple(h for h in _COVSEL_HIST if not (nodual and h in ("dnorm", "derr")))
        res = _stack_fits(per, hist)
        for key in ("xopt", "zopt", "uopt"):
            res[key] = res[key].reshape((n, n, K), order="F")
        res["jacobi_sweeps"] = np.array([r["engine_info"]["jacobi_sweeps"] for r in per], dtype=np.int64)
    else:
        from .covsel_multi import CovselMulti
        obj = CovselMulti(lam, D=D, S=S, device=int(options.get("device", 0)))
        res = _run_and_close(obj, rhos=rhos, nodualerror=nodual, check_every=int(options.get("check_every", 0)),
                             **starts, **loop)
    res["lams"] = lam.copy()
    res["rhos"] = rhos.copy()
    res["solverruntime"] = time.perf_counter() - t0
    return res


def _covsel_single_S(S, lam, options):
    """``covarianceselection`` on a given S (the per-fit route of covarianceselection_multi for n > 96)"""
    t0 = time.perf_counter()
    options = dict(options)
    n = S.shape[0]
    args = _engine_args(options, dict(S=S))
    args["lambda"] = lam
    minx, minz, _ = getproxops("CovarianceSelection", args)
    options.update(A=1, B=-1, c=0, m=n, nA=n, nB=n, obj=_ENGINE_OBJ)
    results = admm(minx, minz, options)
    for key in ("xopt", "zopt", "uopt", "x0", "z0", "u0"):
        if key in results:
            results[key] = np.asarray(results[key]).reshape((n, n), order="F")
    results["solverruntime"] = time.perf_counter() - t0
    return results


def covarianceselection_path(D, lams=None, options=None):
    """results = covarianceselection_path(D, lams, options): the regularisation path of covariance selection, every
    lambda side by side in one run of ``covarianceselection_multi``.  ``lams = None``:
    ``options['nlambda']`` values (default 10), log-spaced from lambda_max = max over i != j of |S_ij| -- at and above it
    the fit is diagonal -- down to ``options['lambda_min_ratio']`` * lambda_max (default 1e-2), with S = cov(D) formed on
    the host.  Returns covarianceselection_multi's fields plus ``df``: per fit the number of pairs i < j with
    z_ij != 0, the edges of the selected graph."""
    options = _options(options, "Argument options is not a struct!", optional=True)
    def lambda_max():
        lmax = covarianceselection_lambda_max(D, {"S": options["S"]} if "S" in options else None)
        if not lmax > 0:
            raise ValueError("lambda_max is 0 (S is diagonal): there is no path to follow; pass lams")
        return lmax

    res = covarianceselection_multi(D, _lambda_grid(options, lams, 10, lambda_max), options)
    res["df"] = covsel_df(res["zopt"])
    return res


def covsel_df(zopt):
    """per fit of an n x n x K array the number of off-diagonal pairs i < j with z_ij != 0"""
    Z = np.asarray(zopt)
    Z = Z.reshape(Z.shape[0], Z.shape[1], -1)
    iu = np.triu_indices(Z.shape[0], k=1)
    return np.count_nonzero(Z[iu[0], iu[1], :], axis=0).astype(np.int64)
