"""The reference's testers (/root/reference/testers/*.m) on top of the device solvers.

``[results, test] = xxxtest(seed, rows, cols, errtol, quiet, options)``: generate the tester's random
problem (``synth.py`` restates each recipe with NumPy's RNG: MATLAB's streams cannot be reproduced),
run the solver on the GPU and evaluate the tester's own pass criterion.  ``test['failed']`` is 0/1
exactly as the reference sets it; the other ``test`` fields carry the quantities the criterion used.
Plots (``showresults``) are not part of the engine.
"""
from __future__ import annotations

import numpy as np

from . import solvers, synth

__all__ = ["lassotest", "sparselassotest", "grouplassotest", "elasticnettest", "ladtest", "quantileregtest", "quantileregmultitest", "sparsequantileregtest", "huberfittest", "totalvariationtest", "linearsvmtest", "sparsesvmtest", "l1classifiertest", "basispursuittest",
           "linearprogramtest", "modeltest", "covarianceselectiontest", "covarianceselectionpathtest", "sparselassocvtest", "sparsel1classifiercvtest", "solvertester"]


def _opts(options, **forced):
    o = dict(options or {})
    o.update(forced)
    return o


def lassotest(seed=0, rows=2 ** 8, cols=2 ** 6, errtol=1e-3, quiet=1, options=None):
    """testers/lassotest.m:31-178: pass when obj(xopt) < obj(testx) (line 143)."""
    p = synth.lasso_problem(seed, rows, cols)
    D, s, lam, testx = p["D"], p["s"], p["lam"], p["testx"]
    obj = lambda x, z: 0.5 * np.sum((D @ x - s) ** 2) + lam * np.sum(np.abs(z))
    results = solvers.lasso(D, s, lam, _opts(options, objevals=1, quiet=quiet))
    xopt = results["xopt"]
    testobj, objopt = obj(testx, testx), obj(xopt, xopt)
    test = dict(D=D, s=s, testx=testx, testobj=testobj, xopt=xopt, admmopt=results["objopt"], objopt=objopt,
                failed=int(not objopt < testobj), objerror=abs((testobj - objopt) / objopt), steps=results["steps"])
    test["lambda"] = lam
    return results, test


def grouplassotest(seed=0, rows=2 ** 8, cols=2 ** 6, errtol=1e-3, quiet=1, options=None):
    """lassotest's shape for grouplasso, on synth.grouplasso_problem (a group-sparse truth): pass when
    obj(xopt) < obj(testx) with obj = 1/2*||D*x - s||^2 + lambda*sum_g ||x_g||_2."""
    p = synth.grouplasso_problem(seed, rows, cols)
    D, s, lam, testx, sizes = p["D"], p["s"], p["lam"], p["testx"], p["groups"]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    pen = lambda z: sum(float(np.linalg.norm(z[a:b])) for a, b in zip(offs[:-1], offs[1:]))
    obj = lambda x, z: 0.5 * np.sum((D @ x - s) ** 2) + lam * pen(z)
    results = solvers.grouplasso(D, s, lam, sizes, _opts(options, objevals=1, quiet=quiet))
    xopt = results["xopt"]
    testobj, objopt = obj(testx, testx), obj(xopt, xopt)
    test = dict(D=D, s=s, testx=testx, groups=sizes, testobj=testobj, xopt=xopt, admmopt=results["objopt"], objopt=objopt,
                failed=int(not objopt < testobj), objerror=abs((testobj - objopt) / objopt), steps=results["steps"])
    test["lambda"] = lam
    return results, test


def sparselassotest(seed=0, rows=2 ** 10, cols=2 ** 8, density=0.05, errtol=1e-3, quiet=1, options=None):
    """lassotest's shape for lasso on a sparse design matrix (synth.sparse_lasso_problem, D a scipy.sparse matrix that
    stays sparse on the device): pass when obj(xopt) < obj(testx)."""
    p = synth.sparse_lasso_problem(seed, rows, cols, density)
    D, s, lam, testx = p["D"], p["s"], p["lam"], p["testx"]
    obj = lambda x, z: 0.5 * np.sum((D @ x - s) ** 2) + lam * np.sum(np.abs(z))
    results = solvers.lasso(D, s, lam, _opts(options, objevals=1, quiet=quiet))
    xopt = results["xopt"]
    testobj, objopt = obj(testx, testx), obj(xopt, xopt)
    test = dict(D=D, s=s, testx=testx, testobj=testobj, xopt=xopt, admmopt=results["objopt"], objopt=objopt,
                failed=int(not objopt < testobj), objerror=abs((testobj - objopt) / objopt), steps=results["steps"],
                nnz=results["nnz"])
    test["lambda"] = lam
    return results, test


def elasticnettest(seed=0, rows=2 ** 8, cols=2 ** 6, ridge=0.5, errtol=1e-3, quiet=1, options=None):
    """lassotest's shape for elasticnet, on lassotest's problem: pass when obj(xopt) < obj(testx) with
    obj = 1/2*||D*x - s||^2 + lambda*||x||_1 + ridge/2*||x||^2."""
    p = synth.lasso_problem(seed, rows, cols)
    D, s, lam, testx = p["D"], p["s"], p["lam"], p["testx"]
    obj = lambda x, z: 0.5 * np.sum((D @ x - s) ** 2) + lam * np.sum(np.abs(z)) + 0.5 * ridge * np.sum(z * z)
    results = solvers.elasticnet(D, s, lam, ridge, _opts(options, objevals=1, quiet=quiet))
    xopt = results["xopt"]
    testobj, objopt = obj(testx, testx), obj(xopt, xopt)
    test = dict(D=D, s=s, testx=testx, ridge=ridge, testobj=testobj, xopt=xopt, admmopt=results["objopt"], objopt=objopt,
                failed=int(not objopt < testobj), objerror=abs((testobj - objopt) / objopt), steps=results["steps"])
    test["lambda"] = lam
    return results, test


def ladtest(seed=0, rows=2 ** 10, cols=2 ** 7, errtol=1e-5, quiet=1, options=None):
    """testers/ladtest.m:37-200: ||xtrue - xopt||_2 < errtol and |objopt - trueobjopt| <= errtol*trueobjopt (149)."""
    p = synth.lad_problem(seed, rows, cols)
    D, s, xtrue = p["D"], p["s"], p["xtrue"]
    results = solvers.lad(D, s, _opts(options, objevals=1, convtest=1, quiet=quiet))
    xopt = results["xopt"]
    trueobj, objopt = np.sum(np.abs(D @ xtrue - s)), np.sum(np.abs(D @ xopt - s))
    xres = np.linalg.norm(xtrue - xopt)
    test = dict(D=D, s=s, truexopt=xtrue, trueobjopt=trueobj, xopt=xopt, admmopt=results["objopt"], objopt=objopt,
                xresidual=xres, xerror=np.sum(np.abs(xtrue - xopt)) / xopt.size,
                failed=int(not (xres < errtol and abs(objopt - trueobj) <= errtol * trueobj)),
                steps=results["steps"], errtol=errtol)
    return results, test


# quantileregtest's allowance on the count condition, in observations: ADMM stops at the default tolerances, not at the
# optimum (tests/test_loss_host.py measures 0 on this problem for tau = 0.1, 0.5, 0.9 and asserts it there)
QUANTILE_COUNT_SLACK = 0


def quantile_count_slack(z, tau):
    """by how many observations #(z < 0) <= tau*m <= #(z < 0) + #(z == 0) fails on z (0: it holds)"""
    z = np.asarray(z).reshape(-1)
    neg, zero, target = int(np.sum(z < 0)), int(np.sum(z == 0)), tau * z.size
    return max(0.0, neg - target, target - (neg + zero))


def quantileregtest(seed=0, rows=200, cols=8, tau=0.9, quiet=1, options=None):
    """ladtest's shape for quantilereg on synth.quantile_problem (D spans the constant vector): pass when the final z
    satisfies the optimality condition on the signs of the residuals, #(z < 0) <= tau*m <= #(z < 0) + #(z == 0), within
    QUANTILE_COUNT_SLACK observations."""
    p = synth.quantile_problem(seed, rows, cols)
    D, s = p["D"], p["s"]
    results = solvers.quantilereg(D, s, tau, _opts(options, objevals=1, quiet=quiet))
    xopt, z = results["xopt"], np.asarray(results["zopt"]).reshape(-1)
    r = D @ xopt - s
    objopt = float(np.sum(tau * np.maximum(r, 0.0) + (1.0 - tau) * np.maximum(-r, 0.0)))
    slack = quantile_count_slack(z, tau)
    test = dict(D=D, s=s, tau=tau, xopt=xopt, admmopt=results["objopt"], objopt=objopt, negative=int(np.sum(z < 0)),
                zero=int(np.sum(z == 0)), slack=slack, failed=int(slack > QUANTILE_COUNT_SLACK), steps=results["steps"])
    return results, test


def quantileregmultitest(seed=0, rows=200, cols=8, taus=(0.1, 0.25, 0.5, 0.75, 0.9), quiet=1, options=None):
    """quantileregtest for quantilereg_multi: the quantiles ``taus`` of synth.quantile_problem (an intercept column) in
    one run; pass when, for every tau, #(z < 0) <= tau*m <= #(z <= 0) holds on that fit's final z within
    QUANTILE_COUNT_SLACK observations.  Returns the ``test`` dict alone; the solver's results are ``test['results']``."""
    p = synth.quantile_problem(seed, rows, cols)
    D, s = p["D"], p["s"]
    results = solvers.quantilereg_multi(D, s, taus, _opts(options, objevals=1, quiet=quiet))
    Z = np.asarray(results["zopt"])
    slack = [quantile_count_slack(Z[:, k], float(tau)) for k, tau in enumerate(taus)]
    test = dict(D=D, s=s, taus=tuple(float(t) for t in taus), xopt=results["xopt"], admmopt=results["objopt"],
                negative=[int(np.sum(Z[:, k] < 0)) for k in range(len(taus))],
                zero=[int(np.sum(Z[:, k] == 0)) for k in range(len(taus))], slack=slack,
                failed=int(any(v > QUANTILE_COUNT_SLACK for v in slack)), steps=results["steps"], results=results)
    return test


def sparsequantileregtest(seed=0, rows=2 ** 10, cols=2 ** 6, density=0.05, taus=(0.1, 0.25, 0.5, 0.75, 0.9), quiet=1,
                          options=None):
    """quantileregmultitest on a sparse design matrix: the quantiles ``taus`` of
    synth.sparse_regression_problem (a dense intercept column among sparse ones) in one run of quantilereg_multi on the
    scipy.sparse D; pass when, for every tau, #(z < 0) <= tau*m <= #(z <= 0) holds on that fit's final z within
    QUANTILE_COUNT_SLACK observations.  Returns the ``test`` dict alone; the solver's results are ``test['results']``."""
    p = synth.sparse_regression_problem(seed, rows, cols, density)
    D, s = p["D"], p["s"]
    results = solvers.quantilereg_multi(D, s, taus, _opts(options, objevals=1, quiet=quiet))
    Z = np.asarray(results["zopt"])
    slack = [quantile_count_slack(Z[:, k], float(tau)) for k, tau in enumerate(taus)]
    test = dict(D=D, s=s, taus=tuple(float(t) for t in taus), xopt=results["xopt"], admmopt=results["objopt"],
                negative=[int(np.sum(Z[:, k] < 0)) for k in range(len(taus))],
                zero=[int(np.sum(Z[:, k] == 0)) for k in range(len(taus))], slack=slack,
                failed=int(any(v > QUANTILE_COUNT_SLACK for v in slack)), steps=results["steps"], results=results)
    return test


def sparselassopathtest(seed=0, rows=2 ** 10, cols=2 ** 8, density=0.05, nlambda=10, quiet=1, options=None):
    """The lasso's regularisation path on a sparse design matrix: lasso_path on
    synth.sparse_lasso_path_problem over ``nlambda`` values, the first one 1.25*lambda_max and the others log-spaced from
    0.8*lambda_max down to 0.01*lambda_max, all in one run.  Pass when the fit above lambda_max returns z = 0.0 exactly
    with ||x|| below its own primal tolerance, and the number of nonzeros of z does not shrink as lambda falls.  Returns
    the ``test`` dict alone; the solver's results are ``test['results']``."""
    p = synth.sparse_lasso_path_problem(seed, rows, cols, density)
    D, s, lmax = p["D"], p["s"], p["lmax"]
    lams = lmax * np.concatenate([[1.25], np.logspace(np.log10(0.8), -2.0, int(nlambda) - 1)])
    results = solvers.lasso_path(D, s, lams, _opts(options, objevals=1, quiet=quiet))
    return _path_test(p, lams, results)


def sparselassocvtest(seed=0, rows=2 ** 10, cols=2 ** 8, density=0.05, nfolds=5, nlambda=10, quiet=1, options=None):
    """Cross-validation of the lasso's path on a sparse design matrix: lasso_cv on
    synth.sparse_lasso_path_problem with ``nfolds`` folds over ``nlambda`` values, the first one 1.25*lambda_max and the
    others log-spaced from 0.8*lambda_max down to 0.01*lambda_max -- (nfolds + 1)*nlambda fits in one run.  Pass when
    every fold fit whose lambda lies above the lambda_max of its own training rows predicts 0 on its held-out rows (its
    held-out error is the sum of s^2 there), the held-out weights are the fold sizes, the selected lambda lies inside the
    path (cvm[index_min] < cvm[0]), lam_1se >= lam_min, and the full-data fits meet the path's own criteria.  Returns
    the ``test`` dict alone; the solver's results are ``test['results']``."""
    p = synth.sparse_lasso_path_problem(seed, rows, cols, density)
    D, s, lmax = p["D"], p["s"], p["lmax"]
    lams = lmax * np.concatenate([[1.25], np.logspace(np.log10(0.8), -2.0, int(nlambda) - 1)])
    results = solvers.lasso_cv(D, s, lams, _opts(options, nfolds=int(nfolds), seed=seed, objevals=1, quiet=quiet))
    fold = results["foldid"]
    sizes = np.bincount(fold, minlength=int(nfolds)).astype(np.float64)
    null = np.array([float(np.sum(s[fold == f] ** 2)) for f in range(int(nfolds))])
    weights_ok = bool(np.array_equal(results["heldout_weight"], np.repeat(sizes[:, None], lams.size, axis=1)))
    own = np.array([float(np.max(np.abs(D.T @ (s * (fold != f))))) for f in range(int(nfolds))])
    above = results["fold_lams"] >= own[:, None]  # (F x L: the fold fit's solution is z = 0)
    null_ok = bool(np.all(np.abs(results["heldout_sse"] - null[:, None])[above] <= 1e-12 * np.repeat(
        null[:, None], lams.size, axis=1)[above]))
    selects = bool(results["cvm"][results["index_min"]] < results["cvm"][0]) and results["lam_1se"] >= results["lam_min"]
    path = dict(results)
    path["perr"] = np.full((int(results["steps"][0]), lams.size), np.inf)  # (lasso_cv keeps no histories)
    test = _path_test(p, lams, path)
    zero_x = bool(np.all(results["zopt"][:, 0] == 0.0))
    test.update(results=results, cvm=results["cvm"], cvsd=results["cvsd"], lam_min=results["lam_min"],
                lam_1se=results["lam_1se"], weights_ok=weights_ok, null_ok=null_ok, null_fits=int(above.sum()),
                selects=selects,
                failed=int(not (zero_x and test["support_grows"] and weights_ok and null_ok and selects)))
    return test


def _path_test(p, lams, results):
    """the pass criteria of a regularisation path whose first lambda lies above lambda_max"""
    D, s, lmax = p["D"], p["s"], p["lmax"]
    Z, X = np.asarray(results["zopt"]), np.asarray(results["xopt"])
    df = [int(v) for v in results["df"]]
    last = int(results["steps"][0]) - 1
    zero = bool(np.all(Z[:, 0] == 0.0)) and float(np.linalg.norm(X[:, 0])) < float(results["perr"][last, 0])
    grows = all(b >= a for a, b in zip(df[:-1], df[1:]))
    test = dict(D=D, s=s, testx=p["testx"], lmax=lmax, lams=lams, df=df, xopt=X, admmopt=results["objopt"],
                zero_above_lmax=zero, support_grows=grows, failed=int(not (zero and grows)), steps=results["steps"],
                results=results)
    return test


def lassopathtest(seed=0, rows=2 ** 9, cols=2 ** 7, nlambda=10, quiet=1, options=None):
    """sparselassopathtest on a dense design matrix: lasso_path_dense on synth.lasso_path_problem over
    ``nlambda`` values, the first one 1.25*lambda_max and the others log-spaced from 0.8*lambda_max down to
    0.01*lambda_max, all in one run over one cached inverse.  The pass criteria and the ``test`` dict are those of
    sparselassopathtest."""
    p = synth.lasso_path_problem(seed, rows, cols)
    D, s, lmax = p["D"], p["s"], p["lmax"]
    lams = lmax * np.concatenate([[1.25], np.logspace(np.log10(0.8), -2.0, int(nlambda) - 1)])
    results = solvers.lasso_path_dense(D, s, lams, _opts(options, objevals=1, quiet=quiet))
    return _path_test(p, lams, results)


def grouplassopathtest(seed=0, rows=2 ** 9, cols=2 ** 7, group=8, nlambda=10, quiet=1, options=None):
    """The group lasso's regularisation path: grouplasso_path on synth.lasso_path_problem's dense matrix
    with a group-sparse truth (every fourth group of ``group`` coefficients live) over ``nlambda`` values, the first one
    1.25*lambda_max and the others log-spaced from 0.8*lambda_max down to 0.01*lambda_max, all in one run.  Pass when
    every block is 0.0 exactly at the lambda above lambda_max, the number of live groups does not shrink as lambda falls,
    and groups enter whole: in every fit a group's block is either all zero or has no zero in it."""
    p = synth.lasso_path_problem(seed, rows, cols)
    D = p["D"]
    sizes = np.full(cols // group, group, dtype=np.int64)
    sizes[-1] += cols - int(sizes.sum())
    rng = np.random.default_rng(seed + 15485863)
    live = np.repeat(np.arange(sizes.size) % 4 == 0, sizes)
    testx = np.where(live, rng.choice([-1.0, 1.0], cols) * rng.uniform(1.0, 3.0, cols), 0.0)
    s = D @ testx + np.sqrt(0.001) * rng.standard_normal(rows)
    lmax = solvers._group_lambda_max(D, s, sizes, None)
    lams = lmax * np.concatenate([[1.25], np.logspace(np.log10(0.8), -2.0, int(nlambda) - 1)])
    results = solvers.grouplasso_path(D, s, sizes, lams, _opts(options, objevals=1, quiet=quiet))
    Z = np.asarray(results["zopt"])
    nz = np.add.reduceat(Z != 0, np.concatenate([[0], np.cumsum(sizes)[:-1]]), axis=0)
    whole = bool(np.all((nz == 0) | (nz == sizes[:, None])))
    dfg = [int(v) for v in results["df_groups"]]
    zero = bool(np.all(Z[:, 0] == 0.0))
    grows = all(b >= a for a, b in zip(dfg[:-1], dfg[1:]))
    return dict(D=D, s=s, testx=testx, groups=sizes, lmax=lmax, lams=lams, df_groups=dfg, xopt=np.asarray(results["xopt"]),
                admmopt=results["objopt"], zero_above_lmax=zero, groups_grow=grows, groups_enter_whole=whole,
                failed=int(not (zero and grows and whole)), steps=results["steps"], results=results)


def huberfittest(seed=0, rows=2 ** 11, cols=2 ** 7, errtol=1e-3, quiet=1, options=None):
    """testers/huberfittest.m:43-188: ADMM's objective is below the planted solution's (line 154)."""
    p = synth.huber_problem(seed, rows, cols)
    D, s, testx = p["D"], p["s"], p["testx"]
    hub = lambda r: np.where(np.abs(r) <= 1.0, r * r, 2.0 * np.abs(r) - 1.0)  # CVX huber
    obj = lambda x: 0.5 * np.sum(hub(D @ x - s))
    results = solvers.huberfit(D, s, _opts(options, objevals=1, convtest=1, quiet=quiet))
    xopt = results["xopt"]
    objoptx, objopt = obj(testx), obj(xopt)
    test = dict(D=D, s=s, testx=testx, xopt=xopt, objoptx=objoptx, objopt=objopt, admmopt=results["objopt"],
                xresidual=np.linalg.norm(xopt - testx), failed=int(not objopt < objoptx), steps=results["steps"],
                errtol=errtol)
    return results, test


def totalvariationtest(seed=0, rows=2 ** 7, errtol=0.02, quiet=1, options=None):
    """testers/totalvariationtest.m:35-190: ADMM's objective is below that of the noise-free signal (line 151)."""
    p = synth.tv_problem(seed, rows)
    s, lam, truex = p["s"], p["lam"], p["truex"]
    obj = lambda x: 0.5 * np.sum((x - s) ** 2) + lam * np.sum(np.abs(np.diff(x)))
    results = solvers.totalvariation(s, lam, _opts(options, objevals=1, maxiters=10000, quiet=quiet))
    xopt = results["xopt"]
    trueobj, objopt = obj(truex), obj(xopt)
    test = dict(s=s, truexopt=truex, trueobjopt=trueobj, xopt=xopt, admmopt=results["objopt"], objopt=objopt,
                failed=int(not objopt < trueobj), relerror=abs((trueobj - objopt) / objopt), steps=results["steps"],
                errtol=errtol)
    test["lambda"] = lam
    return results, test


def linearsvmtest(seed=0, mpos=2 ** 7, mneg=2 ** 7, sep=0.2, errtol=0.05, quiet=1, C=0.5, options=None):
    """testers/linearsvmtest.m:47-280: both runs (lossfunction 'hinge', then the string '0-1' -- which is not
    '01', so the hinge prox runs with the 0-1 objective: getProxOps.m:1094, linearsvm.m:231-237) must beat the
    objective of the true separator [1; -1] and recover its slope to errtol (lines 180, 188)."""
    p = synth.svm_problem(seed, mpos, mneg, sep)
    D, ell = p["D"], p["ell"]
    truex = np.array([1.0, -1.0])
    trueobj = 0.5 * np.sum(truex ** 2) + C * np.sum(np.maximum(np.sign(1.0 - ell * (D @ truex)), 0.0))
    base = _opts(options, objevals=1, convtest=1, quiet=quiet, x0=p["x0"], z0=p["z0"], u0=p["u0"])
    out_r, out_t = {}, {}
    for key, loss in (("hingeloss", "hinge"), ("zoloss", "0-1")):
        r = solvers.linearsvm(D, ell, C, dict(base, lossfunction=loss))
        x = r["xopt"]
        if loss == "hinge":
            objopt = 0.5 * np.sum(x ** 2) + C * np.sum(np.maximum(1.0 - ell * (D @ x), 0.0))
        else:
            objopt = 0.5 * np.sum(x ** 2) + C * np.sum(np.maximum(np.sign(1.0 - ell * (D @ x)), 0.0))
        relerr = abs(1.0 - (-x[1] / x[0]))
        out_r[key] = r
        out_t[key] = dict(truexopt=truex, trueobjopt=trueobj, xopt=x, admmopt=r["objopt"], objopt=objopt,
                          failed=int(not (objopt < trueobj and relerr <= errtol)), relerror=relerr,
                          xresidual=np.linalg.norm(x - truex), steps=r["steps"], errtol=errtol)
    return out_r, out_t


def sparsesvmtest(seed=0, rows=2 ** 10, cols=2 ** 7, density=0.05, classes=3, errtol=0.25, quiet=1, options=None):
    """linearsvmtest's shape for linearsvm_ovr on a sparse design matrix (synth.sparse_svm_problem, D a scipy.sparse
    matrix that stays sparse on the device): the one-vs-rest prediction argmax_c (D*xopt)[:, c] must reproduce the
    planted labels on at least 1 - errtol of the training rows."""
    p = synth.sparse_svm_problem(seed, rows, cols, density, classes)
    D, labels = p["D"], p["labels"]
    results = solvers.linearsvm_ovr(D, labels, p["C"], _opts(options, objevals=1, quiet=quiet,
                                                             classes=np.arange(float(classes))))
    pred = np.argmax(D @ results["xopt"], axis=1).astype(np.float64)
    accuracy = float(np.mean(pred == labels))
    test = dict(D=D, labels=labels, xopt=results["xopt"], accuracy=accuracy, failed=int(not accuracy >= 1.0 - errtol),
                steps=results["steps"], nnz=results["nnz"], cg_capped_updates=results["cg_capped_updates"], errtol=errtol)
    return results, test


def l1classifiertest(seed=0, rows=2 ** 9, cols=2 ** 7, errtol=0.15, quiet=1, options=None):
    """lassotest's shape for l1classifier (l1-regularised logistic regression on synth.sparse_classifier_problem, at a
    tenth of lambda_max): pass when the objective at the sparse iterate z2 lies below the objective of x = 0 -- what
    every lambda >= lambda_max returns -- and sign(D*z2) reproduces the labels on at least 1 - errtol of the rows."""
    p = synth.sparse_classifier_problem(seed, rows, cols)
    D, ell = p["D"], p["ell"]
    o = _opts(options, objevals=1, quiet=quiet)
    Cv = float(o.get("C", 1.0))
    lam = 0.1 * solvers.l1classifier_lambda_max(D, ell, o)
    obj = lambda x: Cv * np.sum(np.logaddexp(0.0, -ell * (D @ x))) + lam * np.sum(np.abs(x))
    results = solvers.l1classifier(D, ell, lam, o)
    z2 = results["zopt"][rows:]
    objopt, zeroobj = obj(z2), obj(np.zeros(cols))
    accuracy = float(np.mean(np.where(D @ z2 >= 0, 1.0, -1.0) == ell))
    test = dict(D=D, ell=ell, testx=p["testx"], xopt=results["xopt"], zopt=z2, admmopt=results["objopt"], objopt=objopt,
                zeroobj=zeroobj, accuracy=accuracy, df=int(np.count_nonzero(z2)),
                failed=int(not (objopt < zeroobj and accuracy >= 1.0 - errtol)), steps=results["steps"], errtol=errtol)
    test["lambda"] = lam
    return results, test


def sparsel1classifiertest(seed=0, rows=2 ** 10, cols=2 ** 8, density=0.05, errtol=0.15, quiet=1, options=None):
    """l1classifiertest on a sparse design matrix (synth.sparse_design_classifier_problem; the matrix-free object of
    DESIGN.md q43): the same lambda, the same two pass criteria, and no x-update that hit the inner iteration cap."""
    p = synth.sparse_design_classifier_problem(seed, rows, cols, density)
    D, ell = p["D"], p["ell"]
    o = _opts(options, objevals=1, quiet=quiet)
    Cv = float(o.get("C", 1.0))
    lam = 0.1 * solvers.l1classifier_lambda_max(D, ell, o)
    obj = lambda x: Cv * np.sum(np.logaddexp(0.0, -ell * (D @ x))) + lam * np.sum(np.abs(x))
    results = solvers.l1classifier(D, ell, lam, o)
    z2 = results["zopt"][rows:]
    objopt, zeroobj = obj(z2), obj(np.zeros(cols))
    accuracy = float(np.mean(np.where(D @ z2 >= 0, 1.0, -1.0) == ell))
    ok = objopt < zeroobj and accuracy >= 1.0 - errtol and results["cg_capped_updates"] == 0
    test = dict(D=D, ell=ell, testx=p["testx"], xopt=results["xopt"], zopt=z2, admmopt=results["objopt"], objopt=objopt,
                zeroobj=zeroobj, accuracy=accuracy, df=int(np.count_nonzero(z2)), failed=int(not ok),
                steps=results["steps"], nnz=results["nnz"], cg_capped_updates=results["cg_capped_updates"], errtol=errtol)
    test["lambda"] = lam
    return results, test


def multinomialtest(seed=0, rows=2 ** 10, cols=2 ** 8, density=0.05, classes=4, errtol=0.3, quiet=1, options=None):
    """The multinomial (softmax) model on a sparse design matrix (synth.sparse_multinomial_problem) at
    lambda = 0.1*lambda_max: the objective at the sparse coefficient block lies below the all-zero model's, the training
    accuracy is at least 1 - errtol, the probabilities sum to one, and no x-update hit the inner iteration cap.  Returns the test dict
    (``failed`` 0 | 1; the solver's results under ``results``)."""
    from . import softmax as M
    p = synth.sparse_multinomial_problem(seed, rows, cols, density, classes)
    D, y = p["D"], p["y"]
    o = _opts(options, objevals=1, quiet=quiet)
    o.pop("quiet", None)
    Cv = float(o.get("C", 1.0))
    lam = 0.1 * M.multinomial_lambda_max(D, y, o)
    results = M.multinomial(D, y, lam, o)
    cls, yi = np.unique(y, return_inverse=True)

    def obj(X):
        T = np.asarray(D @ X)
        tm = T.max(axis=1)
        lse = tm + np.log(np.exp(T - tm[:, None]).sum(axis=1))
        return Cv * float(np.sum(lse - T[np.arange(rows), yi])) + lam * float(np.sum(np.abs(X)))

    z2 = results["zopt"][rows:]
    objopt, zeroobj = obj(z2), obj(np.zeros_like(z2))
    proba = M.multinomial_proba(D, z2)
    accuracy = float(np.mean(cls[np.argmax(proba, axis=1)] == y))
    ok = (objopt < zeroobj and accuracy >= 1.0 - errtol and results["cg_capped_updates"] == 0
          and bool(np.all(np.abs(proba.sum(axis=1) - 1.0) <= 1e-12)))
    test = dict(D=D, y=y, W=p["W"], xopt=results["xopt"], zopt=z2, admmopt=results["objopt"], objopt=objopt,
                zeroobj=zeroobj, accuracy=accuracy, df=int(np.count_nonzero(np.any(z2 != 0, axis=1))), failed=int(not ok),
                steps=results["steps"], nnz=results["nnz"], cg_capped_updates=results["cg_capped_updates"], errtol=errtol)
    test["lambda"] = lam
    test["results"] = results
    return test


def groupclassifiertest(seed=0, rows=2 ** 10, variables=12, levels=6, used=4, sparse=True, errtol=0.15, quiet=1,
                        options=None):
    """Group-lasso logistic regression on one-hot data: ``variables`` categorical variables of ``levels``
    levels each, one-hot coded into variables*levels columns behind a column of ones (the intercept: a group of one with
    weight 0); the labels follow a model that uses the first ``used`` variables alone.  groupclassifier at a fifth of
    groupclassifier_lambda_max with groupweights sqrt(levels), on a scipy.sparse D (``sparse``) or a dense one.  The
    criterion is on recovered groups: every used variable's group has a nonzero in z2, no more than a quarter of the
    unused variables' groups have one, and sign(D*z2) reproduces the labels on at least 1 - errtol of the rows."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed + 4800)
    cat = rng.integers(0, levels, (rows, variables))
    n = 1 + variables * levels
    col = 1 + cat + levels * np.arange(variables)[None, :]
    D = sp.csc_matrix((np.ones(rows * variables), (np.repeat(np.arange(rows), variables), col.reshape(-1))), shape=(rows, n))
    D = sp.csc_matrix(sp.hstack([sp.csc_matrix(np.ones((rows, 1))), D[:, 1:]]))
    truth = np.zeros(n)
    for v in range(used):
        eff = rng.choice([-1.0, 1.0], levels) * rng.uniform(1.0, 2.0, levels)
        truth[1 + v * levels:1 + (v + 1) * levels] = eff - eff.mean()
    score = D @ truth
    ell = np.where(score + 0.1 * float(np.std(score)) * rng.standard_normal(rows) >= 0, 1.0, -1.0)
    sizes = np.array([1] + [levels] * variables, dtype=np.int64)
    gw = np.concatenate([[0.0], np.full(variables, np.sqrt(levels))])
    o = _opts(options, objevals=1, quiet=quiet, groupweights=gw)
    Dd = D if sparse else np.asfortranarray(D.toarray())
    lam = 0.2 * solvers.groupclassifier_lambda_max(Dd, ell, sizes, o)
    results = solvers.groupclassifier(Dd, ell, lam, sizes, o)
    z2 = results["zopt"][rows:]
    alive = np.array([bool(np.any(z2[1 + v * levels:1 + (v + 1) * levels] != 0)) for v in range(variables)])
    accuracy = float(np.mean(np.where(D @ z2 >= 0, 1.0, -1.0) == ell))
    ok = alive[:used].all() and alive[used:].sum() <= (variables - used) // 4 and accuracy >= 1.0 - errtol
    test = dict(D=Dd, ell=ell, testx=truth, groups=sizes, groupweights=gw, xopt=results["xopt"], zopt=z2, alive=alive,
                used_found=int(alive[:used].sum()), unused_found=int(alive[used:].sum()), accuracy=accuracy,
                failed=int(not ok), steps=results["steps"], errtol=errtol)
    test["lambda"] = lam
    return results, test


def sparsel1classifiercvtest(seed=0, rows=2 ** 10, cols=2 ** 8, density=0.05, nfolds=5, nlambda=8, errtol=0.2, quiet=1,
                             options=None):
    """Cross-validation of the l1-regularised logistic regression's path on a sparse design matrix:
    l1classifier_cv on synth.sparse_design_classifier_problem with ``nfolds`` folds over ``nlambda`` values, the first one
    1.25*lambda_max and the others log-spaced from 0.8*lambda_max down to 0.01*lambda_max -- (nfolds + 1)*nlambda fits
    in one run.  Pass when the held-out weights are the fold sizes, every fold fit whose lambda lies 1 % above the
    lambda_max of its own training rows predicts 0 on its held-out rows (a deviance of log 2 per row, every row an
    error), the selected
    lambda lies inside the path (cvm[index_min] < cvm[0]), lam_1se >= lam_min, the held-out error rate at lam_min is at
    most ``errtol``, and no x-update hit the inner iteration cap.  Returns the ``test`` dict alone; the solver's results
    are ``test['results']``."""
    p = synth.sparse_design_classifier_problem(seed, rows, cols, density)
    D, ell = p["D"], p["ell"]
    o = _opts(options, nfolds=int(nfolds), seed=seed, objevals=1, quiet=quiet)
    o.pop("quiet", None)
    lmax = solvers.l1classifier_lambda_max(D, ell)
    lams = lmax * np.concatenate([[1.25], np.logspace(np.log10(0.8), -2.0, int(nlambda) - 1)])
    results = solvers.l1classifier_cv(D, ell, lams, o)
    fold = results["foldid"]
    sizes = np.bincount(fold, minlength=int(nfolds)).astype(np.float64)
    L = lams.size
    full = np.repeat(sizes[:, None], L, axis=1)
    weights_ok = bool(np.array_equal(results["heldout_weight"], full))
    own = np.array([0.5 * float(np.max(np.abs(D.T @ (ell * (fold != f))))) for f in range(int(nfolds))])
    above = results["fold_lams"] >= 1.01 * own[:, None]  # (F x L: the fold fit's solution is z2 = 0)
    null_ok = bool(above.any() and np.all(np.abs(results["heldout_loss"] - np.log(2.0) * full)[above] <= 1e-12 * full[above])
                   and np.array_equal(results["heldout_errors"][above], full[above]))
    selects = bool(results["cvm"][results["index_min"]] < results["cvm"][0]) and results["lam_1se"] >= results["lam_min"]
    rate = float(results["heldout_errors"][:, results["index_min"]].sum() / sizes.sum())
    capped = int(np.sum(results["cg_capped_updates"]))
    ok = weights_ok and null_ok and selects and rate <= errtol and capped == 0
    return dict(results=results, cvm=results["cvm"], cvsd=results["cvsd"], lam_min=results["lam_min"],
                lam_1se=results["lam_1se"], df=results["df"], error_rate=rate, weights_ok=weights_ok, null_ok=null_ok,
                selects=selects, cg_capped_updates=capped, errtol=errtol, failed=int(not ok))


def basispursuittest(seed=0, rows=2 ** 6, cols=2 ** 7, errtol=1e-3, quiet=1, options=None):
    """testers/basispursuittest.m:32-175: ||xopt||_1 <= ||testx||_1 and mean relative residual <= errtol (139)."""
    p = synth.basispursuit_problem(seed, rows, cols)
    D, s, testx = p["D"], p["s"], p["testx"]
    results = solvers.basispursuit(D, s, _opts(options, objevals=1, quiet=quiet, maxiters=10000))
    xopt = results["xopt"]
    Dx = D @ xopt
    relerr = float(np.mean(np.abs((Dx - s) / Dx)))
    test = dict(D=D, s=s, testx=testx, xopt=xopt, objopt=np.sum(np.abs(xopt)), testobj=np.sum(np.abs(testx)),
                relerror=relerr,
                failed=int(not (np.sum(np.abs(testx)) >= np.sum(np.abs(xopt)) and relerr <= errtol)),
                steps=results["steps"])
    return results, test


def linearprogramtest(seed=0, rows=2 ** 6, cols=2 ** 7, errtol=1e-3, quiet=1, options=None):
    """testers/linearprogramtest.m:31-170: objective within errtol of the planted one and D*x = s to errtol (130)."""
    p = synth.lp_problem(seed, rows, cols)
    b, D, s, truex = p["b"], p["D"], p["s"], p["truex"]
    results = solvers.linearprogram(b, D, s, _opts(options, objevals=1, quiet=quiet, maxiters=10000))
    xopt = results["xopt"]
    Dx = D @ xopt
    relerr = float(np.mean(np.abs((Dx - s) / Dx)))
    trueobj, objopt = float(b @ truex), float(b @ xopt)
    test = dict(b=b, D=D, s=s, truexopt=truex, xopt=xopt, trueobjopt=trueobj, objopt=objopt, admmopt=results["objopt"],
                relerror=relerr, objerror=abs((trueobj - objopt) / objopt),
                failed=int(not (abs((trueobj - objopt) / objopt) <= errtol and relerr <= errtol)),
                steps=results["steps"])
    return results, test


def modeltest(seed=0, rows=2 ** 7, cols=2 ** 7, errtol=1e-3, quiet=1, options=None):
    """testers/modeltest.m:37-222: closed form x* = (P'P + Q'Q) \\ (P'r + Q's); objective and x within errtol (122, 156)."""
    p = synth.model_problem(seed, rows, cols)
    P, Q, r, s = p["P"], p["Q"], p["r"], p["s"]
    o = _opts(options, objevals=1, quiet=quiet, maxiters=10000, convtest=1, stopcond="both")
    results = solvers.model(P, Q, r, s, o)
    xt = np.linalg.solve(P.T @ P + Q.T @ Q, P.T @ r + Q.T @ s)
    obj = lambda x: 0.5 * np.sum((P @ x - r) ** 2) + 0.5 * np.sum((Q @ x - s) ** 2)
    xopt = results["xopt"]
    test = dict(P=P, Q=Q, r=r, s=s, truex=xt, xopt=xopt, trueobj=obj(xt), objopt=obj(xopt),
                objerror=abs(1.0 - obj(xopt) / obj(xt)), xerror=np.linalg.norm(xt - xopt),
                failed=int(not (abs(1.0 - obj(xopt) / obj(xt)) <= errtol and np.linalg.norm(xt - xopt) <= errtol)),
                steps=results["steps"])
    return results, test


def covarianceselectiontest(seed=0, rows=2 ** 9, cols=2 ** 6, errtol=1e-3, quiet=1, options=None):
    """testers/covarianceselectiontest.m:91-150: pass when obj(xopt, xopt) < obj(Sinv, Sinv), obj built on the TRUE S
    (not on cov(D)).  q28: line 107 calls errorcheck() without arguments when options.lambda is set, an error in the
    reference; here options['lambda'] is taken."""
    opts = dict(options or {})
    lam = float(opts.get("lambda", 1.0))
    p = synth.covsel_problem(seed, rows, cols)
    S, Sinv = p["S"], p["Sinv"]
    obj = lambda X, Z: np.trace(S @ X) - np.log(np.linalg.det(X)) + lam * np.sum(np.abs(Z))
    results = solvers.covarianceselection(p["D"], lam, _opts(opts, objevals=1, maxiters=1000, convtest=1, quiet=quiet))
    xopt = results["xopt"]
    trueobj, objopt = obj(Sinv, Sinv), obj(xopt, xopt)
    test = dict(D=p["D"], S=S, Sinv=Sinv, trueobjopt=trueobj, xopt=xopt, admmopt=results["objopt"], objopt=objopt,
                failed=int(not objopt < trueobj), objerror=abs((trueobj - objopt) / objopt), steps=results["steps"],
                errtol=errtol)
    test["lambda"] = lam
    return results, test


def covarianceselectionpathtest(seed=0, rows=2 ** 9, cols=2 ** 5, nlambda=6, lambda_min_ratio=0.2, errtol=1e-3, quiet=1,
                                options=None):
    """The regularisation path of covarianceselectiontest's problem through ``covarianceselection_path``:
    ``nlambda`` values log-spaced from 1.25*lambda_max down to ``lambda_min_ratio`` times that, lambda_max = max over
    i != j of |cov(D)_ij|.  Passes when the first fit's Z is exactly diagonal, ``df`` does not decrease as lambda falls,
    and every fit meets covarianceselectiontest's criterion at its own lambda: obj(xopt, xopt) < obj(Sinv, Sinv) on the
    TRUE S.  The grid ends at 0.2 of its top because that criterion judges a fit to cov(D) on the true S: below about
    0.1*lambda_max the penalty no longer covers the sampling noise of 512 rows (|cov(D) - S| ~ 1/sqrt(rows)), and the
    exact minimiser of the sampled problem itself loses to Sinv there (seen on the CPU oracle, seeds 0-4)."""
    opts = dict(options or {})
    p = synth.covsel_problem(seed, rows, cols)
    S, Sinv = p["S"], p["Sinv"]
    lmax = solvers.covarianceselection_lambda_max(p["D"])
    lams = 1.25 * lmax * np.logspace(0.0, np.log10(float(lambda_min_ratio)), int(nlambda))
    results = solvers.covarianceselection_path(p["D"], lams, _opts(opts, objevals=1, maxiters=1000, quiet=quiet))
    obj = lambda X, Z, lam: np.trace(S @ X) - np.log(np.linalg.det(X)) + lam * np.sum(np.abs(Z))
    trueobj = np.array([obj(Sinv, Sinv, lam) for lam in lams])
    objopt = np.array([obj(results["xopt"][:, :, k], results["xopt"][:, :, k], lam) for k, lam in enumerate(lams)])
    Z0 = results["zopt"][:, :, 0]
    diagonal = bool(np.all(Z0 == np.diag(np.diag(Z0))))
    df = results["df"]
    monotone = bool(np.all(np.diff(df) >= 0))
    worse = ~(objopt < trueobj)
    test = dict(D=p["D"], S=S, Sinv=Sinv, lams=lams, lambda_max=lmax, trueobjopt=trueobj, objopt=objopt,
                admmopt=results["objopt"], df=df, diagonal_at_top=diagonal, df_monotone=monotone,
                objerror=np.abs((trueobj - objopt) / objopt), steps=results["steps"], errtol=errtol,
                failed=int(not diagonal) + int(not monotone) + int(np.count_nonzero(worse)))
    return results, test


def _sizes(solver, scale, options):
    """Default scalers of testers/solvertester.m (343-361, 396-408, 480-492, 583-595): problem size per scale."""
    scaler = options.get("scaler")
    if callable(scaler):
        m, n = scaler(scale)
        return int(m), int(n)
    ttype = options.get("testtype", "default")
    if solver == "model":
        if ttype == "fat":
            return 2 ** (scale - 1), 2 ** scale
        if ttype == "skinny":
            return 2 ** scale, 2 ** (scale - 1)
        return 2 ** scale, 2 ** scale
    if solver in ("basispursuit", "linearprogram"):
        n = 2 ** scale
        return -(-n // 5), n
    if solver == "totalvariation":
        return 2 ** scale, 1
    # lasso, lad, huberfit: skinny (8x more rows) unless asked otherwise
    if ttype == "fat":
        return max(1, 2 ** (scale - 3)), 2 ** scale
    if ttype == "square":
        return 2 ** scale, 2 ** scale
    return 2 ** scale, max(1, 2 ** (scale - 3))


def solvertester(solver="model", minscale=2, maxscale=8, trials=10, showplots=0, options=None):
    """results = solvertester(solver, minscale, maxscale, trials, showplots, options)
    (testers/solvertester.m:29-275): run the solver's tester `trials` times at every scale from minscale to
    maxscale (problem sizes 2^scale by the reference's default scalers) and collect runtimes and failures.
    ``showplots`` is accepted and ignored (plots are not part of the engine)."""
    options = dict(options or {})
    tests = {"model": modeltest, "basispursuit": basispursuittest, "linearprogram": linearprogramtest,
             "lasso": lassotest, "totalvariation": totalvariationtest, "lad": ladtest, "huberfit": huberfittest}
    if solver not in tests:
        raise ValueError("Given solver is not a supported solver to test!")
    if not (int(minscale) >= 1 and int(maxscale) >= int(minscale) and int(trials) >= 1):
        raise ValueError("minscale, maxscale and trials must be positive integers with maxscale >= minscale!")
    if "errtol" not in options:  # solvertester.m:93-101
        options["errtol"] = 1e-10 if solver in ("basispursuit", "linearprogram") else 1e-3
    seed_rng = np.random.default_rng(options.get("seed"))
    passthrough = {k: v for k, v in options.items() if k not in ("errtol", "testtype", "scaler", "seed")}
    nscale = int(maxscale) - int(minscale) + 1
    runtimes = np.zeros((nscale, int(trials)))
    failed = np.zeros((nscale, int(trials)), dtype=int)
    steps = np.zeros((nscale, int(trials)), dtype=int)
    seeds = np.zeros((nscale, int(trials)), dtype=np.int64)
    for r, scale in enumerate(range(int(minscale), int(maxscale) + 1)):
        m, n = _sizes(solver, scale, options)
        for c in range(int(trials)):
            seed = int(seed_rng.integers(0, 2 ** 31 - 1))
            if solver == "totalvariation":
                res, test = tests[solver](seed, m, options["errtol"], 1, passthrough)
            else:
                res, test = tests[solver](seed, m, n, options["errtol"], 1, passthrough)
            seeds[r, c] = seed
            runtimes[r, c] = res["solverruntime"]
            failed[r, c] = test["failed"]
            steps[r, c] = res["steps"]
    return dict(solver=solver, scales=list(range(int(minscale), int(maxscale) + 1)), runtimes=runtimes, failed=failed,
                steps=steps, seeds=seeds, avetimes=runtimes.mean(axis=1), failure=int(failed.any()), errtol=options["errtol"])
