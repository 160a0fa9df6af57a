"""The path and cross-validation front ends of solvers.py and softmax.py without a device: with the multi-fit runner behind
each of them replaced by a recorder, what they hand to it -- the automatic lambda grid, the checked lambda vector, the
(F + 1)*L layout of a cross-validation -- and what they cut out of its result; and, with a fake owner, the order in which
the two runners apply their setters.  Every expected value is written out here from the documented formula."""
import importlib
import re

import numpy as np
import pytest
import scipy.sparse as sp

M, N, F, L = 12, 5, 3, 2
_RNG = np.random.default_rng(5)
DENSE = np.asfortranarray(_RNG.standard_normal((M, N)))
SPARSE = sp.csc_matrix(np.where(np.abs(DENSE) > 0.3, DENSE, 0.0))
RESP = _RNG.standard_normal(M)
ELL = np.array([1.0, -1.0, 1.0, -1.0, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0, -1.0, 1.0])
LABELS = np.array([0, 1, 2, 0, 1, 2, 2, 1, 0, 0, 1, 2])
GROUPS = np.array([2, 1, 2], dtype=np.int64)
FOLD = np.array([0, 1, 2, 2, 1, 0, 0, 1, 2, 1, 0, 2])
WEIGHTS = np.array([1.0, 2.0, 1.0, 0.5, 1.0, 3.0, 1.0, 1.5, 1.0, 1.0, 2.5, 1.0])
LAMS = np.array([0.4, 0.1])
NZ = np.array([1, 2, 3, 4, 5, 0, 2, 4])  # the nonzero coefficients of fit k in a synthetic result (k mod 8)

# (two of the messages in two pieces each: a search of the tree for either shows its one home in solvers.py)
BAD_COUNT = "options.nlambda must be " + "an integer >= 1"
BAD_RATIO = "options.lambda_min_ratio must lie in (0, 1]"
NO_LAMBDA = "lams must hold at " + "least one lambda"


def raises(message):
    return pytest.raises(ValueError, match="^" + re.escape(message) + "$")


def synthetic(K, rows, row0, held=()):
    """a multi-fit result whose entry for fit k encodes k; the coefficient block of zopt starts at ``row0`` and holds
    NZ[k mod 8] nonzeros in fit k, the rows above it are all nonzero"""
    k = np.arange(K)
    Z = np.zeros((rows, K), order="F")
    Z[:row0] = k + 1.0
    for j in range(K):
        Z[row0:row0 + NZ[j % 8], j] = j + 1.0
    res = dict(xopt=np.asfortranarray(1000.0 + k[None, :] + 0.01 * np.arange(rows - row0)[:, None]), zopt=Z,
               uopt=np.asfortranarray(-Z - 1.0), steps=100 + k, objopt=k + 0.5, nnz=7, cg_iters_total=11 + k,
               cg_capped_updates=0 * k, chunk=10, runtime=0.25, xsolve="cg")
    for i, key in enumerate(held):
        res[key] = 1.0 + (k % 3) if key == "heldout_weight" else 10.0 * (i + 1) + k * k
    return res


@pytest.fixture
def rec(ap, monkeypatch):
    """replaces the four multi-fit runners by recorders of (lams, options, groups); returns the list of calls"""
    solvers, softmax = ap.solvers, importlib.import_module(ap.__name__ + ".softmax")
    calls = []

    def note(lams, options, groups=None):
        calls.append(dict(lams=np.array(lams, dtype=np.float64).reshape(-1), options=dict(options), groups=groups))
        return calls[-1]["lams"]

    def run_multi_lasso(D, S, lams, options, who, sparse, t0, groups=None):
        lam = note(lams, options, groups)
        res = synthetic(lam.size, N, 0, ("heldout_sse", "heldout_weight") if "heldout" in options else ())
        res["lams"] = lam.copy()
        return res

    def run_multi_classifier(D, ELL, lams, options, who, t0, groups=None):
        lam = note(lams, options, groups)
        res = synthetic(lam.size, M + N, M,
                        ("heldout_loss", "heldout_errors", "heldout_weight") if "heldout" in options else ())
        res["lams"] = lam.copy()
        return res

    def covsel_multi(D, lams, options=None):
        lam = note(lams, options)
        return dict(zopt=np.zeros((N, N, lam.size)), lams=lam.copy())

    def run_models(D, y, lams, options, who, t0):
        lam = note(lams, options)
        return [dict(xopt=np.zeros((N, 3)), zopt=np.zeros((M + N, 3)), uopt=np.zeros((M + N, 3)), classes=np.arange(3),
                     steps=2, lam=float(v), objopt=0.5, nnz=7, cg_iters_total=3, cg_capped_updates=0, runtime=0.25)
                for v in lam]

    monkeypatch.setattr(solvers, "_run_multi_lasso", run_multi_lasso)
    monkeypatch.setattr(solvers, "_run_multi_classifier", run_multi_classifier)
    monkeypatch.setattr(solvers, "covarianceselection_multi", covsel_multi)
    monkeypatch.setattr(softmax, "_run_models", run_models)
    return calls


# ------------------------------------------------------------------------------------------------ the entry points
def _group_norms(g):
    first = np.concatenate([[0], np.cumsum(GROUPS)])
    return np.array([np.sqrt(np.sum(g[a:b] * g[a:b])) for a, b in zip(first[:-1], first[1:])])


def _lmax_lasso(D):  # max_i |(D's)_i|
    return float(np.abs(np.asarray(D.T @ RESP.reshape(-1, 1))).max())


def _lmax_classifier(D, weights=None):  # C*|phi'(0)|*max_j |sum_i c_i*ell_i*D_ij|, logistic: 1/2
    return 0.5 * float(np.abs(np.asarray(D.T @ ((np.ones(M) if weights is None else weights) * ELL))).max())


def _lmax_covsel():  # max over i != j of |cov(D)_ij|
    C = np.cov(DENSE, rowvar=False)
    C = 0.5 * (C + C.T)
    return float(np.abs(C - np.diag(np.diag(C))).max())


def _lmax_multinomial():  # max over classes c and columns j of |sum_i D_ij*(1/Cn - [y_i = c])|
    R = 1.0 / 3 - (LABELS[:, None] == np.arange(3)[None, :])
    return float(np.abs(np.asarray(SPARSE.T @ R)).max())


# name: (call(ap, lams, options), lambda_max, a scalar lams is a count, the default count, cross-validation)
ENTRY = {
    "lasso_path": (lambda ap, lams, o: ap.lasso_path(SPARSE, RESP, lams, o), lambda: _lmax_lasso(SPARSE), False, 10, False),
    "lasso_path_dense": (lambda ap, lams, o: ap.solvers.lasso_path_dense(DENSE, RESP, lams, o), lambda: _lmax_lasso(DENSE),
                         False, 10, False),
    "grouplasso_path": (lambda ap, lams, o: ap.grouplasso_path(DENSE, RESP, GROUPS, lams, o),
                        lambda: float(_group_norms(DENSE.T @ RESP).max()), False, 10, False),
    "l1classifier_path": (lambda ap, lams, o: ap.l1classifier_path(SPARSE, ELL, lams, o), lambda: _lmax_classifier(SPARSE),
                          True, 10, False),
    "groupclassifier_path": (lambda ap, lams, o: ap.solvers.groupclassifier_path(DENSE, ELL, GROUPS, lams, o),
                             lambda: 0.5 * float(_group_norms(DENSE.T @ ELL).max()), True, 10, False),
    "covarianceselection_path": (lambda ap, lams, o: ap.covarianceselection_path(DENSE, lams, o), _lmax_covsel, False, 10,
                                 False),
    "multinomial_path": (lambda ap, lams, o: importlib.import_module(ap.__name__ + ".softmax").multinomial_path(
        SPARSE, LABELS, lams, o), _lmax_multinomial, True, 6, False),
    "lasso_cv": (lambda ap, lams, o: ap.lasso_cv(SPARSE, RESP, lams, dict(o, nfolds=F, foldid=FOLD)),
                 lambda: _lmax_lasso(SPARSE), False, 10, True),
    "l1classifier_cv": (lambda ap, lams, o: ap.l1classifier_cv(SPARSE, ELL, lams, dict(o, nfolds=F, foldid=FOLD)),
                        lambda: _lmax_classifier(SPARSE), True, 10, True),
    "groupclassifier_cv": (lambda ap, lams, o: ap.solvers.groupclassifier_cv(SPARSE, ELL, GROUPS, lams,
                                                                             dict(o, nfolds=F, foldid=FOLD)),
                           lambda: 0.5 * float(_group_norms(np.asarray(SPARSE.T @ ELL)).max()), True, 10, True),
}


def _grid(rec, count):
    """the lambdas of the last recorded call: all of them, or behind the fold fits of a cross-validation"""
    assert "nlambda" not in rec[-1]["options"] and "lambda_min_ratio" not in rec[-1]["options"]
    return rec[-1]["lams"][-count:]


@pytest.mark.parametrize("name", ENTRY)
def test_the_automatic_grid(ap, rec, name):
    call, lmax_of, scalar_is_count, default, cv = ENTRY[name]
    lmax = lmax_of()
    call(ap, None, dict(nlambda=1))
    assert np.array_equal(_grid(rec, 1), [lmax]) and rec[-1]["lams"].size == (F + 1 if cv else 1)
    res = call(ap, None, dict(nlambda=4, lambda_min_ratio=0.1))
    want = lmax * np.logspace(0, -1, 4)
    assert np.array_equal(_grid(rec, 4), want) and rec[-1]["lams"].size == (4 * (F + 1) if cv else 4)
    assert np.array_equal(res["lams"], want)
    call(ap, None, dict(nlambda=np.int64(3)))  # the default ratio
    assert np.array_equal(_grid(rec, 3), lmax * np.logspace(0, -2, 3))
    call(ap, None, {})
    assert np.array_equal(_grid(rec, default), lmax * np.logspace(0, -2, default))
    # lams given: handed on as they are, the two grid options popped and never read
    call(ap, [0.3, 0.2, 0.1], dict(nlambda="never read", lambda_min_ratio=7))
    assert np.array_equal(_grid(rec, 3), [0.3, 0.2, 0.1])
    if scalar_is_count:  # a count beside options.nlambda wins over it
        call(ap, 3, dict(nlambda=5, lambda_min_ratio=0.1))
        assert np.array_equal(_grid(rec, 3), lmax * np.logspace(0, -1, 3))
        for bad in (0, 2.5):
            with raises(BAD_COUNT):
                call(ap, bad, {})
    else:  # one lambda
        call(ap, 3, dict(nlambda=5, lambda_min_ratio=0.1))
        assert np.array_equal(_grid(rec, 1), [3.0]) and rec[-1]["lams"].size == (F + 1 if cv else 1)
    n = len(rec)
    for bad in (0, 2.5, -1, "3"):
        with raises(BAD_COUNT):
            call(ap, None, dict(nlambda=bad))
    for bad in (0, 1.5, "a", -0.1, [0.1]):
        with raises(BAD_RATIO):
            call(ap, None, dict(lambda_min_ratio=bad))
    with raises(BAD_COUNT):  # the count is checked before the ratio
        call(ap, None, dict(nlambda=0, lambda_min_ratio=0))
    assert len(rec) == n  # every refusal before the runner


@pytest.mark.parametrize("name", ENTRY)
def test_true_is_not_a_count(ap, rec, name):
    with raises(BAD_COUNT):
        ENTRY[name][0](ap, None, dict(nlambda=True))
    assert not rec


def test_the_callers_own_checks_around_the_grid(ap, rec):
    for call in (lambda: ap.lasso_path(SPARSE, RESP[:-1], None, dict(nlambda=0)),
                 lambda: ap.solvers.lasso_path_dense(DENSE, RESP[:-1], None, dict(nlambda=0)),
                 lambda: ap.grouplasso_path(DENSE, RESP[:-1], GROUPS, None, dict(nlambda=0))):
        with raises("The number of rows in argument D do not match size of s!"):  # ahead of the count
            call()
    with raises("grouplasso_path: with options.l1 != 0 lambda_max has no closed form: give lams"):
        ap.grouplasso_path(DENSE, RESP, GROUPS, None, dict(l1=0.1, nlambda=0))
    for lams in (None, 3):
        with raises("groupclassifier_path: with options.l1 != 0 lambda_max has no closed form: give lams"):
            ap.solvers.groupclassifier_path(DENSE, ELL, GROUPS, lams, dict(l1=[0.0, 0.1], nlambda=0))
        with raises("groupclassifier_cv: with options.l1 != 0 lambda_max has no closed form: give lams"):
            ap.solvers.groupclassifier_cv(SPARSE, ELL, GROUPS, lams, dict(l1=0.1, nlambda=0))
    assert not rec
    ap.grouplasso_path(DENSE, RESP, GROUPS, [0.2], dict(l1=0.1))  # lams given: l1 is free
    assert len(rec) == 1
    with raises(BAD_COUNT):  # lambda_max is taken after the count and the ratio have passed
        ap.covarianceselection_path(None, None, dict(S=np.eye(4), nlambda=0))
    with raises(BAD_RATIO):
        ap.covarianceselection_path(None, None, dict(S=np.eye(4), lambda_min_ratio=2))
    with raises("lambda_max is 0 (S is diagonal): there is no path to follow; pass lams"):
        ap.covarianceselection_path(None, None, dict(S=np.eye(4)))
    assert len(rec) == 1


def test_lambda_max_under_weights_is_the_grids_first_point(ap, rec):
    ap.lasso_path(SPARSE, RESP, None, dict(nlambda=2, obsweights=WEIGHTS))
    assert _grid(rec, 2)[0] == float(np.abs(np.asarray(SPARSE.T @ (WEIGHTS * RESP).reshape(-1, 1))).max())
    ap.l1classifier_cv(SPARSE, ELL, 2, dict(nfolds=F, foldid=FOLD, weights=WEIGHTS))
    assert _grid(rec, 2)[0] == _lmax_classifier(SPARSE, WEIGHTS)


# ------------------------------------------------------------------------------------------------ the lambda vector
def _stub_owner(ap, monkeypatch, module, cls):
    made = []

    class Owner:
        def __init__(self, *args, **kw):
            made.append(self)

    monkeypatch.setattr(importlib.import_module(ap.__name__ + "." + module), cls, Owner)
    return made


@pytest.mark.parametrize("name", ("lasso_multi", "lasso_multi_dense", "grouplasso_multi", "l1classifier_multi",
                                  "groupclassifier_multi", "multinomial_path", "covarianceselection_multi"))
def test_the_lambda_vector_check(ap, monkeypatch, name):
    softmax = importlib.import_module(ap.__name__ + ".softmax")
    call = dict(lasso_multi=lambda lams: ap.lasso_multi(SPARSE, RESP, lams, {}),
                lasso_multi_dense=lambda lams: ap.solvers.lasso_multi_dense(DENSE, RESP, lams, {}),
                grouplasso_multi=lambda lams: ap.grouplasso_multi(DENSE, RESP, lams, GROUPS, {}),
                l1classifier_multi=lambda lams: ap.l1classifier_multi(SPARSE, ELL, lams, {}),
                groupclassifier_multi=lambda lams: ap.solvers.groupclassifier_multi(DENSE, ELL, lams, GROUPS, {}),
                multinomial_path=lambda lams: softmax.multinomial_path(SPARSE, LABELS, lams, {}),
                covarianceselection_multi=lambda lams: ap.covarianceselection_multi(DENSE, lams, {}))[name]
    made = [_stub_owner(ap, monkeypatch, module, cls)
            for module, cls in (("sparse_lasso", "SparseLassoMulti"), ("lasso_multi", "LassoMulti"),
                                ("sparse_l1class", "SparseL1Classifier"), ("l1class", "L1Classifier"),
                                ("covsel_multi", "CovselMulti"))]
    noun = "model" if name == "multinomial_path" else "fit"
    positive = name == "covarianceselection_multi"
    kind = "positive" if positive else "nonnegative"
    with raises(NO_LAMBDA):
        call([])
    with raises(NO_LAMBDA):
        call(np.zeros((0, 3)))
    for bad, k in (([0.3, -0.1], 1), ([np.nan, 0.2, 0.1], 0), ([0.3, 0.2, np.inf], 2), ([0.3, -np.inf, np.nan], 1),
                   (np.array([[0.3, 0.2], [0.1, -1.0]]), 3)):
        with raises(f"{noun} {k}: lambda is not a {kind} real number"):
            call(bad)
    if positive:
        with raises("fit 1: lambda is not a positive real number"):
            call([0.3, 0.0])
    assert not any(made)  # every refusal before an owner exists


@pytest.mark.parametrize("name", [k for k in ENTRY if k != "covarianceselection_path"])
def test_zero_is_a_lambda(ap, rec, name):
    ENTRY[name][0](ap, [0.3, 0.0], {})
    assert np.array_equal(_grid(rec, 2), [0.3, 0.0])


# ------------------------------------------------------------------------------------------------ the cross-validation
CV = {
    "lasso_cv": dict(call=lambda ap, lams, o: ap.lasso_cv(SPARSE, RESP, lams, o), wkey="obsweights", rows=N, row0=0,
                     held=("heldout_sse", "heldout_weight"), y="s",
                     short=lambda ap: ap.lasso_cv(SPARSE, RESP[:-1], LAMS, {})),
    "l1classifier_cv": dict(call=lambda ap, lams, o: ap.l1classifier_cv(SPARSE, ELL, lams, o), wkey="weights", rows=M + N,
                            row0=M, held=("heldout_loss", "heldout_errors", "heldout_weight"), y="ell",
                            short=lambda ap: ap.l1classifier_cv(SPARSE, ELL[:-1], LAMS, {})),
    "groupclassifier_cv": dict(call=lambda ap, lams, o: ap.solvers.groupclassifier_cv(SPARSE, ELL, GROUPS, lams, o),
                               wkey="weights", rows=M + N, row0=M,
                               held=("heldout_loss", "heldout_errors", "heldout_weight"), y="ell",
                               short=lambda ap: ap.solvers.groupclassifier_cv(SPARSE, ELL[:-1], GROUPS, LAMS, {})),
}


def _fold_lams(scale=True):
    total = WEIGHTS.sum()
    train = np.array([total - WEIGHTS[FOLD == f].sum() for f in range(F)])
    return (train / total if scale else np.ones(F))[:, None] * LAMS[None, :]


@pytest.mark.parametrize("name", CV)
def test_cv_layout(ap, rec, name):
    c = CV[name]
    x0 = np.arange(N * L, dtype=np.float64).reshape(N, L)
    z0 = np.arange(c["rows"] * L, dtype=np.float64).reshape(c["rows"], L) + 0.5
    u0 = -np.asfortranarray(z0)
    o = {c["wkey"]: WEIGHTS, "nfolds": F, "foldid": FOLD, "ridge": [0.1, 0.2], "nonnegative": np.array([0, 1]),
         "x0": x0, "z0": z0, "u0": u0, "abstol": 1e-9, "nlambda": 3, "seed": 8}
    if name == "groupclassifier_cv":
        o["l1"] = (0.3, 0.4)
    given = dict(o)
    got = c["call"](ap, LAMS, o)
    assert len(rec) == 1 and set(o) == set(given) and all(o[k] is given[k] for k in o)  # ONE run; the caller's dict is whole
    sent, lams = rec[0]["options"], rec[0]["lams"]
    want = _fold_lams()
    assert 0.0 < want[0, 0] < LAMS[0] and len(set(want[:, 0])) == F  # non-uniform weights: every fold its own fraction
    assert np.array_equal(lams[:F * L], want.reshape(-1)) and np.array_equal(lams[F * L:], LAMS) and lams.size == (F + 1) * L
    assert list(sent["heldout"]) == [0, 0, 1, 1, 2, 2, -1, -1] and np.array_equal(sent["foldid"], FOLD)
    assert sent["foldid"].dtype == np.int64
    assert list(sent["ridge"]) == [0.1, 0.2] * (F + 1) and list(sent["nonnegative"]) == [0, 1] * (F + 1)
    if name == "groupclassifier_cv":
        assert list(sent["l1"]) == [0.3, 0.4] * (F + 1) and np.array_equal(rec[0]["groups"], GROUPS)
    for key, v in (("x0", x0), ("z0", z0), ("u0", u0)):
        assert np.array_equal(sent[key], np.tile(v, (1, F + 1))) and sent[key].flags["F_CONTIGUOUS"], key
        assert np.array_equal(sent[key][:, 2 * L:3 * L], v)
    assert sent["abstol"] == 1e-9 and sent[c["wkey"]] is WEIGHTS
    for key in ("nfolds", "seed", "scale_lambda", "measure", "nlambda", "lambda_min_ratio"):
        assert key not in sent, key
    # what comes back: fit f*L + l is fold f at lambda l, the fits from F*L on see every row
    k = np.arange(F * L)
    ref = synthetic((F + 1) * L, c["rows"], c["row0"], c["held"])
    for key in c["held"]:
        assert np.array_equal(got[key], ref[key][:F * L].reshape(F, L)), key
        assert got[key][1, 0] == ref[key][2]
    assert np.array_equal(got["fold_steps"], (100 + k).reshape(F, L)) and np.array_equal(got["fold_lams"], want)
    assert list(got["steps"]) == [106, 107] and list(got["objopt"]) == [6.5, 7.5]
    for key in ("xopt", "zopt", "uopt"):
        assert np.array_equal(got[key], ref[key][:, F * L:]) and got[key].flags["F_CONTIGUOUS"], key
    assert got["xopt"][0, 1] == 1007.0
    assert list(got["df"]) == [2, 4] and got["df"].dtype == np.int64  # NZ[6], NZ[7]: the coefficient block alone
    summary = ap.solvers.cv_summary(got[c["held"][0]], got["heldout_weight"], LAMS)
    sums = (10.0 + k * k).reshape(F, L)
    assert np.array_equal(summary["cvm"], sums.sum(axis=0) / (1.0 + (k % 3)).reshape(F, L).sum(axis=0))
    for key, v in summary.items():
        assert np.array_equal(got[key], v), key
    keys = {"lams", "foldid", "cvm", "cvsd", "index_min", "lam_min", "index_1se", "lam_1se", "xopt", "zopt", "uopt", "df",
            "steps", "objopt", "fold_steps", "fold_lams", "nnz", "cg_iters_total", "cg_capped_updates", "chunk", "runtime",
            "solverruntime"} | set(c["held"])
    if name != "lasso_cv":
        keys.add("measure")
        assert got["measure"] == "deviance"
    if name == "groupclassifier_cv":
        keys |= {"groups", "df_groups"}
        assert list(got["df_groups"]) == [1, 3] and got["df_groups"].dtype == np.int64  # 2 of [2|1|2], 4 of [2|1|2]
        assert np.array_equal(got["groups"], GROUPS)
    assert set(got) == keys
    assert np.array_equal(got["lams"], LAMS) and np.array_equal(got["foldid"], FOLD)
    assert got["nnz"] == 7 and got["chunk"] == 10 and got["runtime"] == 0.25
    assert np.array_equal(got["cg_iters_total"], 11 + np.arange((F + 1) * L))
    if name != "lasso_cv":
        cls = c["call"](ap, LAMS, dict(nfolds=F, foldid=FOLD, measure="class"))
        assert cls["measure"] == "class"
        for key, v in ap.solvers.cv_summary(cls["heldout_errors"], cls["heldout_weight"], LAMS).items():
            assert np.array_equal(cls[key], v), key
        assert not np.array_equal(cls["cvm"], got["cvm"])


@pytest.mark.parametrize("name", CV)
def test_cv_unscaled_folds_default_folds_and_scalars(ap, rec, name):
    c = CV[name]
    got = c["call"](ap, LAMS, {c["wkey"]: WEIGHTS, "nfolds": F, "foldid": FOLD, "scale_lambda": 0, "ridge": 0.25,
                               "nonnegative": True})
    assert np.array_equal(rec[-1]["lams"], np.tile(LAMS, F + 1)) and np.array_equal(got["fold_lams"], np.tile(LAMS, (F, 1)))
    assert rec[-1]["options"]["ridge"] == 0.25 and rec[-1]["options"]["nonnegative"] is True  # scalars stay scalars
    assert "x0" not in rec[-1]["options"] and "z0" not in rec[-1]["options"]
    got = c["call"](ap, LAMS, dict(nfolds=4, seed=9))
    want = ap.solvers.cv_folds(M, 4, 9)
    assert np.array_equal(got["foldid"], want) and np.array_equal(rec[-1]["options"]["foldid"], want)
    assert np.array_equal(want, np.random.default_rng(9).permutation(M) % 4)
    assert list(rec[-1]["options"]["heldout"]) == [0, 0, 1, 1, 2, 2, 3, 3, -1, -1]
    train = np.array([M - np.count_nonzero(want == f) for f in range(4)])  # no weights: ones
    assert np.array_equal(got["fold_lams"], (train / float(M))[:, None] * LAMS[None, :])
    got = c["call"](ap, LAMS, {})
    assert np.array_equal(got["foldid"], ap.solvers.cv_folds(M, 5, 0)) and got["fold_lams"].shape == (5, L)


@pytest.mark.parametrize("name", CV)
def test_cv_refusals(ap, rec, name):
    c = CV[name]
    call = lambda o, lams=LAMS: c["call"](ap, lams, o)
    for bad in (1, 2.0, True, "3"):
        with raises("options.nfolds must be an integer >= 2"):
            call(dict(nfolds=bad))
    with raises(f"options.heldout is {name}'s own to set: give options.foldid"):
        call(dict(heldout=[0, -1]))
    for bad in (FOLD - 1, FOLD + 1):
        with raises(f"options.foldid: every fold id must lie in [0, nfolds = {F})"):
            call(dict(nfolds=F, foldid=bad))
    with raises(f"The number of rows in argument D do not match size of {c['y']}!"):
        c["short"](ap)
    with raises(NO_LAMBDA):
        call({}, [])
    with raises(f"options.{c['wkey']}: the total weight must be positive"):
        call({c["wkey"]: np.zeros(M)})
    for key in ("ridge", "nonnegative") + (("l1",) if name == "groupclassifier_cv" else ()):
        with raises(f"{key} has 3 entries for {L} lambdas"):
            call({key: [0.0, 0.0, 0.0]})
    for key, rows in (("x0", N), ("z0", c["rows"]), ("u0", c["rows"])):
        for bad in (np.zeros((rows, L + 1)), np.zeros((rows + 1, L)), np.zeros(rows * L)):
            with raises(f"options.{key} is not a {rows} x {L} matrix (one column per lambda)!"):
                call({key: bad})
    if name != "lasso_cv":
        for bad in ("auc", 1, None):
            with raises("options.measure must be 'deviance' or 'class'"):
                call(dict(measure=bad))
        with raises("classcost is one (pos, neg) pair or 'balanced' in l1classifier_cv"):
            call(dict(classcost=np.ones((L, 2))))
        with raises("options.lossfunction is not a string!"):
            call(dict(lossfunction=["hinge", "hinge"]))
    assert not rec  # every refusal before the run
    for fn, args in ((ap.lasso_cv, (DENSE, RESP)), (ap.l1classifier_cv, (DENSE, ELL)),
                     (ap.solvers.groupclassifier_cv, (DENSE, ELL, GROUPS))):
        with pytest.raises(ValueError, match="runs on a scipy.sparse D"):
            fn(*args)


def test_cv_classcost_is_one_pair_from_all_rows(ap, rec):
    ap.l1classifier_cv(SPARSE, ELL, LAMS, dict(nfolds=F, foldid=FOLD, classcost="balanced"))
    assert tuple(rec[-1]["options"]["classcost"]) == (M / (2.0 * 7), M / (2.0 * 5))  # 7 positive, 5 negative of 12
    ap.l1classifier_cv(SPARSE, ELL, LAMS, dict(nfolds=F, foldid=FOLD, classcost=(2.0, 0.5), lossfunction="hinge"))
    assert tuple(rec[-1]["options"]["classcost"]) == (2.0, 0.5) and rec[-1]["options"]["lossfunction"] == "hinge"


# ------------------------------------------------------------------------------------------------ the paths' own keys
def test_the_paths_count_the_coefficient_block(ap, rec):
    lams = np.linspace(0.8, 0.1, 8)
    assert list(ap.lasso_path(SPARSE, RESP, lams, {})["df"]) == list(NZ)
    assert list(ap.solvers.lasso_path_dense(DENSE, RESP, lams, {})["df"]) == list(NZ)
    got = ap.grouplasso_path(DENSE, RESP, GROUPS, lams, {})
    groups_hit = [1, 1, 2, 3, 3, 0, 1, 3]  # the first NZ[k] coefficients of [2 | 1 | 2]
    assert list(got["df"]) == list(NZ) and list(got["df_groups"]) == groups_hit
    assert got["df"].dtype == got["df_groups"].dtype == np.int64 and np.array_equal(rec[-1]["groups"], GROUPS)
    assert list(ap.l1classifier_path(SPARSE, ELL, lams, {})["df"]) == list(NZ)
    got = ap.solvers.groupclassifier_path(SPARSE, ELL, GROUPS, lams, {})
    assert list(got["df"]) == list(NZ) and list(got["df_groups"]) == groups_hit


# ------------------------------------------------------------------------------------------------ the setters' order
def _logged(name):
    def method(self, *args, **kw):
        self.log.append(name)
    return method


class _Owner:
    """an owner without a device that logs the calls it gets"""
    log = None
    set_cost, set_groups, set_folds, set_observations = map(_logged, ("set_cost", "set_groups", "set_folds",
                                                                      "set_observations"))

    def __init__(self, D, Y, lams, *args, **kw):
        self.K = int(np.size(lams))
        self.log.append("init")

    def run(self, **kw):
        self.log.append("run")
        return {}

    def results(self, summary):
        self.log.append("results")
        return dict(steps=np.zeros(self.K, dtype=np.int64))

    def heldout(self):
        self.log.append("heldout")
        return tuple(np.zeros(self.K) for _ in range(self.held))

    def close(self):
        self.log.append("close")


def _owner(ap, monkeypatch, module, cls, held):
    log = []
    monkeypatch.setattr(importlib.import_module(ap.__name__ + "." + module), cls,
                        type("Logged", (_Owner,), dict(log=log, held=held)))
    return log


def test_the_classifier_sets_cost_then_groups_then_folds(ap, monkeypatch):
    log = _owner(ap, monkeypatch, "sparse_l1class", "SparseL1Classifier", 3)
    o = dict(weights=WEIGHTS, classcost=(2.0, 1.0), foldid=FOLD, heldout=[0, -1], l1=[0.1, 0.2], groupweights=[1.0, 0.0, 2.0])
    res = ap.solvers.groupclassifier_multi(SPARSE, ELL, LAMS, GROUPS, o)
    assert log == ["init", "set_cost", "set_groups", "set_folds", "run", "results", "heldout", "close"]
    assert set(res) >= {"heldout_loss", "heldout_errors", "heldout_weight", "groups", "lams", "solverruntime"}
    del log[:]
    ap.l1classifier_multi(SPARSE, ELL, LAMS, dict(foldid=FOLD, heldout=[0, -1]))  # no cost, no groups
    assert log == ["init", "set_folds", "run", "results", "heldout", "close"]
    del log[:]
    ap.solvers.groupclassifier_multi(SPARSE, ELL, LAMS, GROUPS, dict(classcost="balanced"))
    assert log == ["init", "set_cost", "set_groups", "run", "results", "close"]
    del log[:]
    ap.l1classifier_multi(SPARSE, ELL, LAMS, {})
    assert log == ["init", "run", "results", "close"]


def test_the_lasso_sets_groups_then_observations(ap, monkeypatch):
    log = _owner(ap, monkeypatch, "sparse_lasso", "SparseLassoMulti", 2)
    res = ap.grouplasso_multi(SPARSE, RESP, LAMS, GROUPS, dict(obsweights=WEIGHTS, foldid=FOLD, heldout=[1, -1], l1=0.1))
    assert log == ["init", "set_groups", "set_observations", "run", "results", "heldout", "close"]
    assert set(res) >= {"heldout_sse", "heldout_weight", "groups", "lams"}
    del log[:]
    ap.lasso_multi(SPARSE, RESP, LAMS, dict(obsweights=WEIGHTS))
    assert log == ["init", "set_observations", "run", "results", "heldout", "close"]
    del log[:]
    ap.grouplasso_multi(SPARSE, RESP, LAMS, GROUPS, {})
    assert log == ["init", "set_groups", "run", "results", "close"]
    del log[:]
    ap.lasso_multi(SPARSE, RESP, LAMS, {})
    assert log == ["init", "run", "results", "close"]
