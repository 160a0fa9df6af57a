"""The sparse l1 classifier under held-out folds without a device: the numbers test_gpu_sparse_l1class_cv
depends on, computed from the two restatements alone -- the parity gap (MEASURED_GAP), the sensitivity of a held-out
loss sum to zopt (LOSS_CONDITION), and the two conditions under which the weighted errors and the two indices may be
compared exactly -- and the pure arithmetic of l1classifier_cv against a stub owner: the fold-fit layout, the lambda
scaling, the measure, the refusals."""
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

import sparse_l1class_cv_restated as W


def _gap(name, got, ref):
    assert got["steps"] == ref["steps"], (name, got["steps"], ref["steps"])
    assert got["cg_capped_updates"] == 0, name
    gap = W.relgap(got, ref)
    print(f"{name}: steps {ref['steps']}, gap {gap:.3e}")
    return gap


# ------------------------------------------------------------------------------------------------ 1. MEASURED_GAP
@pytest.mark.parametrize("obj", W.OBJECTS)
@pytest.mark.parametrize("shape", W.SHAPES)
def test_gap_per_iteration(ap, shape, obj):
    worst = 0.0
    for nd in (0, 1):
        for k in range(W.K):
            worst = max(worst, _gap(f"{shape} {obj} nd={nd} fit {k}", W.restated_fit(ap, shape, obj, k, W.PARITY_LOOP, nd),
                                    W.restated_fit(ap, shape, obj, k, W.PARITY_LOOP, nd, cholesky=True)))
    print(f"per iteration {shape} {obj}: largest gap {worst:.3e}")
    assert worst <= W.MEASURED_GAP, worst


@pytest.mark.parametrize("shape", W.SHAPES)
def test_gap_free_running_and_the_distinct_stops(ap, shape):
    """nodualerror = 1 from the zero start at the default tolerances (under nodualerror = 0 the small-lambda runs cost the
    restatement 15 - 25 s each: left out, as in test_gpu_sparse_l1class)"""
    worst, steps = 0.0, []
    for k in range(W.K):
        ref = W.restated_fit(ap, shape, "logistic", k, None, 1, free=True)
        worst = max(worst, _gap(f"{shape} free fit {k}", ref,
                                W.restated_fit(ap, shape, "logistic", k, None, 1, free=True, cholesky=True)))
        steps.append(ref["steps"])
    print(f"free-running {shape}: steps {steps}, largest gap {worst:.3e}")
    assert len(set(steps[:W.F * W.L])) >= W.FREE_DISTINCT, steps
    assert worst <= W.MEASURED_GAP, worst


def _edge_cases(ap):
    return [W.edge_case(ap, *W.edge_problem(shape)) for shape in (W.SHAPES[0], W.EDGE_M)]


def test_gap_on_the_edge_folds_and_the_cross_validation(ap):
    worst = 0.0
    for c in _edge_cases(ap):
        shape = c["A"].shape
        for k in range(W.K):
            worst = max(worst, _gap(f"edge {shape} fit {k}", W.edge_fit(ap, c, k), W.edge_fit(ap, c, k, cholesky=True)))
    for f in range(W.CV_FOLDS + 1):
        for l in range(W.CV_NLAMBDA):
            worst = max(worst, _gap(f"cv fold {f} lambda {l}", W.cv_fit(ap, f, l), W.cv_fit(ap, f, l, cholesky=True)))
    print(f"edge folds and cross-validation: largest gap {worst:.3e}")
    assert worst <= W.MEASURED_GAP, worst


def test_the_bound_follows_from_the_measurement():
    assert W.PARITY_BOUND == 10.0 * W.MEASURED_GAP and W.PARITY_BOUND <= 1e-6


# ------------------------------------------------------------------------------------------------ 2. the sensitivity
def _compared_fits(ap):
    """(case, k, reference run, rho) of every fit whose held-out sums the device test compares"""
    rho = W.PARITY_LOOP["rho"]
    for shape in W.SHAPES:
        for obj in W.OBJECTS:
            c = W.case(ap, shape, obj)
            for k in range(W.K):
                yield c, k, W.restated_fit(ap, shape, obj, k, W.PARITY_LOOP, 1), rho
        c = W.case(ap, shape, "logistic")
        for k in range(W.K):
            yield c, k, W.restated_fit(ap, shape, "logistic", k, None, 1, free=True), 1.0
    for c in _edge_cases(ap):
        for k in range(W.K):
            yield c, k, W.edge_fit(ap, c, k), rho


def test_loss_sensitivity_factor(ap):
    worst = max(W.loss_condition(c, k, r["zopt"]) for c, k, r, _ in _compared_fits(ap))
    cv = W.cv_case(ap)
    m, n = cv["A"].shape
    for f in range(W.CV_FOLDS):
        rows = np.flatnonzero(cv["foldid"] == f)
        for l in range(W.CV_NLAMBDA):
            z = W.cv_fit(ap, f, l)["zopt"]
            S = W.heldout_sums(cv["A"], cv["ell"], np.ones(m), "logistic", cv["foldid"], f, z)[0]
            worst = max(worst, float(np.sqrt(rows.size) * np.linalg.norm(cv["A"][rows], 2) * np.sqrt(n) *
                                     np.max(np.abs(z)) / S))
    print(f"loss sensitivity factor {worst:.3e}")
    assert 1.0 <= worst <= W.LOSS_CONDITION


# ------------------------------------------------------------------------------------------------ 3. the two conditions
def test_the_two_conditions_hold(ap):
    """on the reference alone: no held-out row's t_i is within the z bound's reach of 0 unless it is zero by structure,
    and no coefficient within its reach of the soft threshold (sparse_l1class_cv_restated.error_margin): the support of z2
    and the weighted errors are compared exactly; and no two cvm values that decide index_min / index_1se lie closer than
    twice the cvm bound"""
    margin = min(W.fit_margin(c, k, r, rho, W.PARITY_BOUND) for c, k, r, rho in _compared_fits(ap))
    cv = W.cv_case(ap)
    for f in range(W.CV_FOLDS + 1):
        for l in range(W.CV_NLAMBDA):
            lam = float(cv["fold_lams"][f, l]) if f < W.CV_FOLDS else float(cv["lams"][l])
            margin = min(margin, W.error_margin(cv["A"], np.flatnonzero(cv["foldid"] == f), W.cv_fit(ap, f, l), lam, 1.0,
                                                W.PARITY_BOUND))
    print(f"smallest margin over the held-out rows and the coefficients: {margin:.3e}")
    assert margin > 0.0
    loss, err, wt = W.cv_sums(ap)
    for name, sums, tol in (("deviance", loss, W.PARITY_BOUND * W.LOSS_CONDITION), ("class", err, W.PARITY_BOUND)):
        r = ap.solvers.cv_summary(sums, wt, cv["lams"])
        cvm = r["cvm"]
        others = np.delete(cvm, r["index_min"])
        gap_min = float(np.min(np.abs(others - cvm[r["index_min"]])))
        bar = cvm[r["index_min"]] + r["cvsd"][r["index_min"]]
        gap_bar = float(np.min(np.abs(cvm - bar)))
        print(f"{name}: cvm {cvm}, index_min {r['index_min']}, index_1se {r['index_1se']}, gaps {gap_min:.3e} {gap_bar:.3e}")
        # (the bar moves with cvm and cvsd: cvsd is compared at sqrt(2)*tol*max e, a cvm value at tol*cvm)
        reach = 2.0 * tol * float(np.max(cvm)) * (1.0 + np.sqrt(2.0) * float(np.max(sums / wt)) / float(np.max(cvm)))
        assert gap_min > 2.0 * tol * float(np.max(cvm)) and gap_bar > reach, (name, gap_min, gap_bar, reach)


# ------------------------------------------------------------------------------------------------ 4. the pure arithmetic
M, N = 9, 4
DENSE = np.asfortranarray(np.random.default_rng(0).standard_normal((M, N)))
SPARSE = sp.csc_matrix(np.where(np.abs(DENSE) > 0.4, DENSE, 0.0))
ELL = np.array([1.0, -1.0, 1.0, -1.0, 1.0, 1.0, -1.0, -1.0, 1.0])
FOLD = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2])


@pytest.fixture
def stub(ap, monkeypatch):
    """replaces SparseL1Classifier by an owner without a device that records what it was given; returns the list"""
    mod = importlib.import_module(ap.__name__ + ".sparse_l1class")
    made = []

    class Stub(mod.SparseL1Classifier):
        def __init__(self, D, ELL, lams, losses=None, ridge=None, nonnegative=None, l1weights=None, **kw):
            self._h = None
            self.m, self.n = (int(v) for v in D.shape)
            self.lams = np.asarray(lams, dtype=np.float64)
            self.losses, self.ridge = losses, ridge
            self.K, self.nnz, self.closed, self.objevals, self.dual = int(self.lams.size), 7, False, False, True
            self.folds = self.cost = None
            made.append(self)

        @classmethod
        def chunk(cls):
            return 10

        def set_cost(self, weights=None, classcost=None):
            self.cost = (weights, classcost)

        def set_folds(self, fold=None, heldout=None):
            self.folds = (np.asarray(fold), np.asarray(heldout))

        def heldout(self):
            k = np.arange(self.K, dtype=np.float64)
            held = self.folds[1] >= 0
            return np.where(held, 10.0 + k * k, 0.0), np.where(held, 1.0 + (k % 3), 0.0), np.where(held, 3.0, 0.0)

        def run(self, **kw):
            self.run_kw = kw
            self.objevals = bool(kw.get("objevals", 0))
            self.dual = not kw.get("nodualerror", 0)
            return dict(steps=np.arange(self.K, dtype=np.int64) + 2, stopped_early=np.ones(self.K, dtype=np.int64),
                        objopt=np.arange(self.K, dtype=np.float64) + 0.5, runtime=0.25,
                        cg_iters_total=np.arange(self.K, dtype=np.int64) + 11,
                        cg_capped_updates=np.zeros(self.K, dtype=np.int64))

        def fetch(self, field, rows):
            return np.asfortranarray(100.0 * field + np.arange(rows * self.K, dtype=np.float64).reshape(rows, self.K))

        def close(self):
            self.closed = True

    monkeypatch.setattr(mod, "SparseL1Classifier", Stub)
    return made


_MULTI_KEYS = {"xopt", "zopt", "uopt", "steps", "pnorm", "perr", "objopt", "runtime", "solverruntime", "chunk", "lams",
               "xsolve", "nnz", "cg_iters_total", "cg_capped_updates"}


def test_multi_and_path_take_the_two_options_and_add_three_keys(ap, stub):
    plain = ap.l1classifier_multi(SPARSE, ELL, [0.3, 0.2], dict(nodualerror=1))
    assert set(plain) == _MULTI_KEYS and stub[-1].folds is None and stub[-1].closed
    got = ap.l1classifier_multi(SPARSE, ELL, [0.3, 0.2], dict(nodualerror=1, foldid=FOLD, heldout=[1, -1]))
    assert set(got) == _MULTI_KEYS | {"heldout_loss", "heldout_errors", "heldout_weight"}
    assert list(got["heldout_loss"]) == [10.0, 0.0] and list(got["heldout_weight"]) == [3.0, 0.0]
    f, h = stub[-1].folds
    assert f.dtype == h.dtype == np.int32 and list(f) == list(FOLD) and list(h) == [1, -1] and stub[-1].closed
    assert stub[-1].cost is None
    path = ap.l1classifier_path(SPARSE, ELL, [0.3, 0.2], dict(nodualerror=1, foldid=FOLD, heldout=[1, -1],
                                                              weights=np.ones(M)))
    assert set(path) == set(got) | {"df"} and stub[-1].cost[0] is not None and stub[-1].folds is not None


def test_cv_layout_lambda_scaling_and_measure(ap, stub):
    lams = np.array([0.4, 0.2, 0.1, 0.05])
    w = np.array([1.0, 2.0, 1.0, 1.0, 1.0, 3.0, 1.0, 1.0, 1.0])
    got = ap.l1classifier_cv(SPARSE, ELL, lams, dict(nfolds=3, foldid=FOLD, weights=w, classcost="balanced",
                                                     ridge=[0.0, 0.1, 0.2, 0.3], lossfunction="hinge"))
    assert len(stub) == 1 and stub[0].closed  # ONE object
    o = stub[0]
    F, L = 3, 4
    assert o.K == (F + 1) * L
    fold, held = o.folds
    assert list(fold) == list(FOLD) and list(held) == [0] * L + [1] * L + [2] * L + [-1] * L
    train = np.array([w.sum() - w[FOLD == f].sum() for f in range(F)])
    want = (train / w.sum())[:, None] * lams[None, :]
    assert np.array_equal(got["fold_lams"], want) and np.array_equal(o.lams[:F * L], want.reshape(-1))
    assert np.array_equal(o.lams[F * L:], lams) and np.array_equal(got["lams"], lams)
    assert list(o.ridge) == [0.0, 0.1, 0.2, 0.3] * (F + 1) and o.losses == ["hinge"] * o.K
    # 'balanced' from ALL rows: 5 positive, 4 negative of 9, the same pair for every fit
    cc = o.cost[1]
    assert cc.shape == (o.K, 2) and np.all(cc == np.array([9 / 10.0, 9 / 8.0]))
    k = np.arange(F * L, dtype=np.float64)
    assert np.array_equal(got["heldout_loss"], (10.0 + k * k).reshape(F, L))
    assert np.array_equal(got["heldout_errors"], (1.0 + (k % 3)).reshape(F, L)) and np.all(got["heldout_weight"] == 3.0)
    S = ap.solvers.cv_summary
    assert got["measure"] == "deviance"
    for key, v in S(got["heldout_loss"], got["heldout_weight"], lams).items():
        assert np.array_equal(got[key], v), key
    cls = ap.l1classifier_cv(SPARSE, ELL, lams, dict(nfolds=3, foldid=FOLD, measure="class"))
    for key, v in S(cls["heldout_errors"], cls["heldout_weight"], lams).items():
        assert np.array_equal(cls[key], v), key
    assert cls["measure"] == "class" and not np.array_equal(cls["cvm"], got["cvm"])
    # the full-data path is the last L fits
    assert list(got["steps"]) == [14, 15, 16, 17] and got["fold_steps"].shape == (F, L) and got["fold_steps"][1, 2] == 8
    assert got["xopt"].shape == (N, L) and got["zopt"].shape == (M + N, L) and got["df"].shape == (L,)
    assert np.array_equal(got["df"], np.count_nonzero(got["zopt"][M:], axis=0))
    assert got["nnz"] == 7 and got["cg_iters_total"].shape == (o.K,) and got["runtime"] == 0.25 and got["chunk"] == 10
    assert set(got) == {"lams", "foldid", "measure", "cvm", "cvsd", "index_min", "lam_min", "index_1se", "lam_1se", "xopt",
                        "zopt", "uopt", "df", "steps", "objopt", "fold_steps", "fold_lams", "heldout_loss",
                        "heldout_errors", "heldout_weight", "nnz", "cg_iters_total", "cg_capped_updates", "chunk",
                        "runtime", "solverruntime"}
    # scale_lambda = 0: every fold at lambda_l itself; the default folds are cv_folds'
    flat = ap.l1classifier_cv(SPARSE, ELL, lams, dict(nfolds=3, seed=4, scale_lambda=0))
    assert np.array_equal(flat["fold_lams"], np.tile(lams, (3, 1)))
    assert np.array_equal(flat["foldid"], ap.solvers.cv_folds(M, 3, 4)) and stub[-1].cost is None
    # a count, or None: l1classifier_path's grid from the full-data lambda_max
    grid = ap.l1classifier_cv(SPARSE, ELL, 5, dict(nfolds=2, weights=w, lambda_min_ratio=0.1))
    lmax = ap.l1classifier_lambda_max(SPARSE, ELL, dict(weights=w))
    assert grid["lams"].size == 5 and grid["lams"][0] == lmax and grid["lams"][-1] == pytest.approx(0.1 * lmax, rel=1e-14)
    assert ap.l1classifier_cv(SPARSE, ELL, None, dict(nfolds=2))["lams"].size == 10
    z0 = np.arange((M + N) * 4, dtype=np.float64).reshape(M + N, 4)
    ap.l1classifier_cv(SPARSE, ELL, lams, dict(nfolds=3, z0=z0))
    assert np.array_equal(stub[-1].run_kw["z0"], np.tile(z0, (1, 4)))


def test_cv_refusals(ap, stub):
    with pytest.raises(ValueError, match="SparseL1Classifier"):
        ap.l1classifier_cv(DENSE, ELL)
    with pytest.raises(ValueError, match="rows"):
        ap.l1classifier_cv(SPARSE, ELL[:-1])
    for bad in (1, 2.0, True):
        with pytest.raises(ValueError, match="nfolds"):
            ap.l1classifier_cv(SPARSE, ELL, None, dict(nfolds=bad))
    with pytest.raises(ValueError, match="heldout is l1classifier_cv's own"):
        ap.l1classifier_cv(SPARSE, ELL, None, dict(heldout=np.zeros(10)))
    with pytest.raises(ValueError, match="foldid"):
        ap.l1classifier_cv(SPARSE, ELL, None, dict(nfolds=2, foldid=FOLD))
    with pytest.raises(ValueError, match="foldid has"):
        ap.l1classifier_cv(SPARSE, ELL, None, dict(foldid=np.zeros(4)))
    with pytest.raises(ValueError, match="measure"):
        ap.l1classifier_cv(SPARSE, ELL, None, dict(measure="auc"))
    with pytest.raises(ValueError, match="nlambda"):
        ap.l1classifier_cv(SPARSE, ELL, 0)
    with pytest.raises(ValueError, match="ridge has 2"):
        ap.l1classifier_cv(SPARSE, ELL, [0.3, 0.2, 0.1], dict(ridge=[0.0, 0.1]))
    with pytest.raises(ValueError, match="z0"):
        ap.l1classifier_cv(SPARSE, ELL, [0.3, 0.2, 0.1], dict(z0=np.zeros((N, 3))))
    with pytest.raises(ValueError, match="lossfunction"):
        ap.l1classifier_cv(SPARSE, ELL, [0.3], dict(lossfunction=["hinge"]))
    with pytest.raises(ValueError, match="options.obsweights"):
        ap.l1classifier_cv(SPARSE, ELL, [0.3], dict(obsweights=np.ones(M)))
    with pytest.raises(ValueError, match="total weight"):
        ap.l1classifier_cv(SPARSE, ELL, [0.3], dict(weights=np.zeros(M)))
    with pytest.raises(TypeError):
        ap.l1classifier_cv(SPARSE, ELL, None, 3)
    assert not stub  # every refusal before an object exists


def test_multi_refusals(ap, stub):
    for call in (lambda o: ap.l1classifier_multi(SPARSE, ELL, [0.1, 0.2], o),
                 lambda o: ap.l1classifier_path(SPARSE, ELL, [0.1, 0.2], o)):
        with pytest.raises(ValueError, match="options.obsweights .* options.weights"):
            call(dict(obsweights=np.ones(M)))
        with pytest.raises(ValueError, match="options.heldout needs options.foldid"):
            call(dict(heldout=[0, -1]))
        with pytest.raises(ValueError, match="options.foldid needs options.heldout"):
            call(dict(foldid=FOLD))
        with pytest.raises(ValueError, match="foldid has 4"):
            call(dict(foldid=FOLD[:4], heldout=[0, -1]))
        with pytest.raises(ValueError, match="heldout has 3"):
            call(dict(foldid=FOLD, heldout=[0, 1, 2]))
        with pytest.raises(ValueError, match="foldid must hold integers"):
            call(dict(foldid=FOLD + 0.5, heldout=[0, -1]))
    assert not stub
    for key, value in (("foldid", FOLD), ("heldout", [0, -1])):  # a dense D: refused by name
        with pytest.raises(ValueError, match=f"options.{key}"):
            ap.l1classifier_multi(DENSE, ELL, [0.1, 0.2], {key: value})


def test_abi_symbols(ap):
    Lm = ap._lib
    lib = Lm.load()
    for name in ("admm_sparse_l1class_set_folds", "admm_sparse_l1class_heldout"):
        assert name in Lm.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.admm_abi_version() == 5
    assert "l1classifier_cv" in ap.solvers.__all__ and ap.l1classifier_cv is ap.solvers.l1classifier_cv
    assert "sparsel1classifiercvtest" in ap.testers.__all__
