"""What the multi-fit solvers hand back, without a device: every owner class is replaced by a stub whose run / fetch
return small known arrays, and the public callers are checked for the exact key set of their result, the history
length, the dropped fit axis of the K = 1 wrappers and the close() of the owner -- also when run raises."""
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

M, N = 5, 4
STEPS = {3: (2, 4, 1), 1: (4,)}
OWNERS = (("engine", "SvmOvr"), ("reg_multi", "RegMulti"), ("sparse_svm", "SparseSvmOvr"),
          ("sparse_reg", "SparseRegMulti"), ("sparse_lasso", "SparseLassoMulti"))
NODUAL_DEFAULT = dict(SparseRegMulti=1, SparseLassoMulti=0)


def _stub(real, K, made, fail):
    class Stub(real):
        def __init__(self, D, *args, **kw):
            self._h = None
            self.m, self.n = (int(v) for v in D.shape)
            self.K, self.nnz = K, 7
            self.closed = False
            self.objevals = False
            made.append(self)

        @classmethod
        def chunk(cls):
            return 10

        def set_weights(self, *args):
            pass

        def set_cost(self, *args):
            pass

        def run(self, **kw):
            if fail:
                raise RuntimeError("the stub's run fails")
            self.objevals = bool(kw.get("objevals", 0))
            if real.__name__ in NODUAL_DEFAULT:
                self.dual = not kw.get("nodualerror", NODUAL_DEFAULT[real.__name__])
            out = dict(steps=np.array(STEPS[K], dtype=np.int64), stopped_early=np.ones(K, dtype=np.int64),
                       objopt=np.arange(K, dtype=np.float64) + 0.5)
            if real.__name__.startswith("Sparse"):
                out.update(cg_iters_total=np.arange(K, dtype=np.int64) + 11,
                           cg_capped_updates=np.zeros(K, dtype=np.int64))
            out["runtime"] = 0.25
            return out

        def fetch(self, field, rows):
            return np.asfortranarray(100.0 * field + np.arange(rows * K, dtype=np.float64).reshape(rows, K))

        def close(self):
            self.closed = True

    Stub.__name__ = real.__name__
    return Stub


@pytest.fixture
def stubbed(ap, monkeypatch):
    """install(K, fail=False) replaces the five owner classes and returns the list every stub made is appended to"""
    def install(K, fail=False):
        made = []
        for module, name in OWNERS:
            mod = importlib.import_module(ap.__name__ + "." + module)
            monkeypatch.setattr(mod, name, _stub(getattr(mod, name), K, made, fail))
        return made
    return install


DENSE = np.asfortranarray(np.random.default_rng(0).standard_normal((M, N)))
SPARSE = sp.csc_matrix(np.where(np.abs(DENSE) > 0.4, DENSE, 0.0))
RESP = np.random.default_rng(1).standard_normal(M)
LABELS = np.array([0.0, 1.0, 2.0, 1.0, 0.0])
ELL = np.array([1.0, -1.0, 1.0, -1.0, 1.0])
FITS = [dict(kind="lad"), dict(kind="lad", tau=0.3), dict(kind="huber", delta=0.7)]

# caller -> (K, honours options.nodualerror, call(ap, options))
CALLERS = {
    "lasso_multi": (3, True, lambda ap, o: ap.lasso_multi(SPARSE, RESP, [0.3, 0.2, 0.1], o)),
    "lasso_path": (3, True, lambda ap, o: ap.lasso_path(SPARSE, RESP, [0.3, 0.2, 0.1], o)),
    "robustfit_multi_dense": (3, False, lambda ap, o: ap.robustfit_multi(DENSE, RESP, FITS, o)),
    "robustfit_multi_sparse": (3, True, lambda ap, o: ap.robustfit_multi(SPARSE, RESP, FITS, o)),
    "lad_sparse": (1, True, lambda ap, o: ap.lad(SPARSE, RESP, o)),
    "huberfit_sparse": (1, True, lambda ap, o: ap.huberfit(SPARSE, RESP, o)),
    "linearsvm_ovr_dense": (3, False, lambda ap, o: ap.linearsvm_ovr(DENSE, LABELS, 1.0, o)),
    "linearsvm_ovr_sparse": (3, False, lambda ap, o: ap.linearsvm_ovr(SPARSE, LABELS, 1.0, o)),
    "linearsvm_sparse": (1, False, lambda ap, o: ap.linearsvm(SPARSE, ELL, 1.0, o)),
}

_CORE = {"xopt", "zopt", "uopt", "steps", "pnorm", "perr", "objopt", "runtime", "solverruntime"}
_CG = {"xsolve", "nnz", "cg_iters_total", "cg_capped_updates"}
# the key set of each caller with objevals = 0 and, where the caller honours it, nodualerror = 1: taken from the code
# before the owners shared one result path.  objevals = 1 adds "objevals"; nodualerror = 0 adds "dnorm" and "derr".
BASE_KEYS = {
    "lasso_multi": _CORE | _CG | {"chunk", "lams"},
    "lasso_path": _CORE | _CG | {"chunk", "lams", "df"},
    "robustfit_multi_dense": _CORE | {"chunk", "fallback"},
    "robustfit_multi_sparse": _CORE | _CG | {"chunk"},
    "lad_sparse": _CORE | _CG,
    "huberfit_sparse": _CORE | _CG,
    "linearsvm_ovr_dense": _CORE | {"classes", "Hnormsq"},
    "linearsvm_ovr_sparse": _CORE | _CG | {"classes", "Hnormsq"},
    "linearsvm_sparse": _CORE | _CG | {"Hnormsq"},
}
HISTORIES = ("pnorm", "perr", "dnorm", "derr", "Hnormsq", "objevals")


@pytest.mark.parametrize("nodual", (0, 1))
@pytest.mark.parametrize("objevals", (0, 1))
@pytest.mark.parametrize("caller", sorted(CALLERS))
def test_result_keys_histories_and_close(ap, stubbed, caller, objevals, nodual):
    K, honours, call = CALLERS[caller]
    made = stubbed(K)
    res = call(ap, dict(objevals=objevals, nodualerror=nodual) if honours else dict(objevals=objevals))
    want = set(BASE_KEYS[caller])
    if objevals:
        want.add("objevals")
    if honours and not nodual:
        want |= {"dnorm", "derr"}
    assert set(res) == want, (sorted(set(res) - want), sorted(want - set(res)))
    rows = max(STEPS[K])
    for key in HISTORIES:
        if key in res:
            assert np.shape(res[key]) == ((rows, K) if K > 1 else (rows,)), key
    assert len(made) == 1 and made[0].closed
    if "chunk" in res:
        assert res["chunk"] == 10
    if "nnz" in res:
        assert res["xsolve"] == "cg" and res["nnz"] == 7
    assert res["runtime"] == 0.25 and res["solverruntime"] >= 0.0
    if K > 1:
        assert res["xopt"].shape == (N, K) and res["uopt"].shape[1] == K
        assert np.array_equal(res["steps"], STEPS[K]) and np.array_equal(res["objopt"], np.arange(K) + 0.5)
        # z and u live on the observations, except in the lasso, where they live on the coefficients
        assert res["zopt"].shape == ((N if caller.startswith("lasso") else M), K)
        if "cg_iters_total" in res:
            assert np.array_equal(res["cg_iters_total"], np.arange(K) + 11)


@pytest.mark.parametrize("caller", ("lad_sparse", "huberfit_sparse", "linearsvm_sparse"))
def test_single_fit_wrappers_drop_the_fit_axis(ap, stubbed, caller):
    K, honours, call = CALLERS[caller]
    stubbed(K)
    res = call(ap, dict(objevals=1, nodualerror=0) if honours else dict(objevals=1))
    for key in ("xopt", "zopt", "uopt") + HISTORIES:
        if key in res:
            assert isinstance(res[key], np.ndarray) and res[key].ndim == 1 and res[key].flags.c_contiguous, key
    assert res["xopt"].shape == (N,) and res["zopt"].shape == (M,) and res["uopt"].shape == (M,)
    for key in ("steps", "cg_iters_total", "cg_capped_updates"):
        assert type(res[key]) is int, key
    assert type(res["objopt"]) is float
    assert res["steps"] == 4 and res["cg_iters_total"] == 11 and res["objopt"] == 0.5


@pytest.mark.parametrize("caller", sorted(CALLERS))
def test_the_owner_is_closed_when_run_raises(ap, stubbed, caller):
    K, _, call = CALLERS[caller]
    made = stubbed(K, fail=True)
    with pytest.raises(RuntimeError, match="the stub's run fails"):
        call(ap, {})
    assert len(made) == 1 and made[0].closed
