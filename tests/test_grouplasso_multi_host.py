"""Group lasso, K fits over one D, without a device: the two new callers against stub owners (arguments,
key sets, close), the group lambda_max against the optimality condition of x = 0, the restatement's parity gap measured
again, and the plan of the grouped element kernel through admm_group_multi_plan."""
import ctypes as C
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

import group_multi_restated as R
from test_multi_results_host import _stub

M, N = 6, 5
DENSE = np.asfortranarray(np.random.default_rng(0).standard_normal((M, N)))
SPARSE = sp.csc_matrix(np.where(np.abs(DENSE) > 0.4, DENSE, 0.0))
RESP = np.random.default_rng(1).standard_normal(M)
GROUPS = [2, 1, 2]
_CORE = {"xopt", "zopt", "uopt", "steps", "pnorm", "perr", "objopt", "runtime", "solverruntime", "chunk", "lams"}
_CG = {"xsolve", "nnz", "cg_iters_total", "cg_capped_updates"}


@pytest.fixture
def stubbed(ap, monkeypatch):
    """install(K, fail=False): both lasso owners replaced by test_multi_results_host's stub, which also records the
    arguments of set_groups; returns the list every stub made is appended to"""
    def install(K, fail=False):
        made = []
        for module, name in (("sparse_lasso", "SparseLassoMulti"), ("lasso_multi", "LassoMulti")):
            mod = importlib.import_module(ap.__name__ + "." + module)
            real = getattr(mod, name)
            stub = _stub(real, K, made, fail)

            def set_groups(self, groups=None, groupweights=None, l1=None):
                self.groups = (groups, groupweights, l1)

            def results(self, summ, _real=real):
                res = _real.__mro__[1].results(self, summ)  # _MultiOwner.results: the dense owner adds xsolve itself
                if not self._cg:
                    res["xsolve"] = "inverse"
                return res

            def run(self, _run=stub.run, **kw):
                self.dual = not kw.get("nodualerror", 0)
                return _run(self, **kw)

            stub.set_groups, stub.results, stub.run = set_groups, results, run
            monkeypatch.setattr(mod, name, stub)
        return made
    return install


@pytest.mark.parametrize("nodual", (0, 1))
@pytest.mark.parametrize("objevals", (0, 1))
@pytest.mark.parametrize("D", (DENSE, SPARSE), ids=("dense", "sparse"))
def test_result_keys_groups_and_close(ap, stubbed, D, objevals, nodual):
    made = stubbed(3)
    o = dict(objevals=objevals, nodualerror=nodual, groupweights=[1.0, 2.0, 0.5], l1=[0.0, 0.1, 0.2])
    res = ap.grouplasso_multi(D, RESP, [0.3, 0.2, 0.1], GROUPS, o)
    want = _CORE | {"groups"} | (_CG if sp.issparse(D) else {"xsolve"})
    want |= ({"objevals"} if objevals else set()) | (set() if nodual else {"dnorm", "derr"})
    assert set(res) == want, (sorted(set(res) - want), sorted(want - set(res)))
    assert len(made) == 1 and made[0].closed
    sizes, gw, l1 = made[0].groups
    assert sizes.dtype == np.int64 and list(sizes) == GROUPS and list(gw) == [1.0, 2.0, 0.5] and list(l1) == [0.0, 0.1, 0.2]
    assert list(res["groups"]) == GROUPS and res["zopt"].shape == (N, 3)
    path = ap.grouplasso_path(D, RESP, GROUPS, [0.3, 0.2, 0.1], dict(o, nlambda=7))
    assert set(path) == want | {"df", "df_groups"} and path["df_groups"].shape == (3,) and made[1].closed
    # the ungrouped callers keep their key sets and never set groups
    plain = (ap.lasso_multi if sp.issparse(D) else ap.lasso_multi_dense)(D, RESP, [0.3, 0.2, 0.1], dict(objevals=objevals, nodualerror=nodual))
    assert set(plain) == want - {"groups"} and not hasattr(made[2], "groups")


def test_scalar_l1_default_weights_and_the_automatic_grid(ap, stubbed):
    made = stubbed(3)
    ap.grouplasso_multi(SPARSE, RESP, [0.3, 0.2, 0.1], GROUPS, dict(l1=0.25))
    sizes, gw, l1 = made[0].groups
    assert gw is None and l1 == [0.25] * 3
    stubbed(10)
    made = stubbed(1)  # (the stub's STEPS knows K = 1 and 3)
    res = ap.grouplasso_path(DENSE, RESP, GROUPS, None, dict(nlambda=1))
    g = DENSE.T @ RESP
    assert res["lams"].shape == (1,) and np.isclose(res["lams"][0], max(np.linalg.norm(g[:2]), abs(g[2]), np.linalg.norm(g[3:])))


@pytest.mark.parametrize("D", (DENSE, SPARSE), ids=("dense", "sparse"))
def test_argument_checks_raise_before_an_owner_exists(ap, stubbed, D):
    made = stubbed(3)
    lams = [0.3, 0.2, 0.1]
    for groups, o, part in (([2, 0, 3], {}, "every size must be >= 1"), ([2, 2], {}, "sizes sum to 4"),
                            ([2, 1.5, 1.5], {}, "integer"), (GROUPS, dict(groupweights=[1.0, -1.0, 1.0]), "groupweights"),
                            (GROUPS, dict(groupweights=[1.0, 1.0]), "2 entries for 3 groups"),
                            (GROUPS, dict(l1=[0.1, -0.1, 0.1]), "fit 1"), (GROUPS, dict(l1=[0.1, 0.1]), "l1 has 2 entries for 3 fits"),
                            (GROUPS, dict(ridge=[0.0, 0.0, -1.0]), "fit 2"), (GROUPS, dict(fast=1), "options.fast"),
                            (GROUPS, dict(relax=1.5), "options.relax"), (GROUPS, dict(stopcond="both"), "stopcond")):
        with pytest.raises(ValueError, match=part):
            ap.grouplasso_multi(D, RESP, lams, groups, o)
    with pytest.raises(ValueError, match="give lams"):
        ap.grouplasso_path(D, RESP, GROUPS, None, dict(l1=[0.0, 0.1, 0.0]))
    with pytest.raises(ValueError, match="nlambda"):
        ap.grouplasso_path(D, RESP, GROUPS, None, dict(nlambda=0))
    with pytest.raises(TypeError):
        ap.grouplasso_multi(D, RESP, lams, GROUPS, 3)
    assert not made
    if not sp.issparse(D):
        with pytest.raises(ValueError, match="stays with lasso"):
            ap.grouplasso_multi(np.asfortranarray(DENSE[:3]), RESP[:3], lams, GROUPS, {})


def test_the_owner_is_closed_when_run_raises(ap, stubbed):
    made = stubbed(3, fail=True)
    with pytest.raises(RuntimeError, match="the stub's run fails"):
        ap.grouplasso_multi(DENSE, RESP, [0.3, 0.2, 0.1], GROUPS, {})
    assert len(made) == 1 and made[0].closed and made[0].groups[0] is not None


# ------------------------------------------------------------------------------------------------ lambda_max
@pytest.mark.parametrize("weighted", (False, True))
def test_lambda_max_is_where_the_zero_solution_stops_being_optimal(ap, weighted):
    """x = 0 solves the group lasso iff ||(D's)_g|| <= lambda*omega_g for every g (the subgradient condition at 0)"""
    rng = np.random.default_rng(11)
    D = rng.standard_normal((40, 23))
    s = rng.standard_normal(40)
    sizes = np.array([1, 7, 3, 12], dtype=np.int64)
    gw = np.array([1.5, 0.0, 0.7, 2.0]) if weighted else None  # a group of weight 0 is unpenalised: not part of the rule
    lmax = ap.solvers._group_lambda_max(D, s, sizes, gw)
    g = D.T @ s
    off = np.concatenate([[0], np.cumsum(sizes)])
    norms = np.array([np.linalg.norm(g[off[j]:off[j + 1]]) for j in range(4)])
    w = np.ones(4) if gw is None else gw
    live = w > 0
    assert np.all(norms[live] <= lmax * (1 + 1e-9) * w[live])
    assert np.count_nonzero(norms[live] > lmax * (1 - 1e-3) * w[live]) == 1
    grid = ap.solvers._lambda_grid(dict(nlambda=4, lambda_min_ratio=0.1), None, 10,
                                   lambda: ap.solvers._group_lambda_max(D, s, sizes, gw))
    assert np.allclose(grid, lmax * np.logspace(0, -1, 4)) and grid[0] == lmax


# ------------------------------------------------------------------------------------------------ the parity gap
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("kind,shape", [(kind, shape) for kind in R.KINDS for shape in R.SHAPES[kind]])
def test_restatement_matches_the_reference_and_measures_the_parity_gap(ap, kind, shape, mode):
    """every fit, with nodualerror 0 and 1, every field (dnorm / derr included), no entry excluded"""
    c = R.case(ap, kind, shape, mode)
    worst = 0.0
    for nd in (0, 1):
        steps = []
        for k in range(R.K):
            ref = R.reference_fit(ap, kind, shape, mode, k, nd)
            got = R.restated_fit(kind, c, k, nd)
            assert got["steps"] == ref["steps"], (k, nd, got["steps"], ref["steps"])
            gap = R.relgap(got, ref)
            print(f"{kind} {shape} {mode} nodualerror={nd} fit {k}: steps {ref['steps']}, gap {gap:.3e}")
            steps.append(ref["steps"])
            worst = max(worst, gap)
        assert len(set(steps)) >= 5, steps  # the reference alone stops the fits at different iterations
        assert np.all(R.reference_fit(ap, kind, shape, mode, 4, nd)["zopt"] == 0.0)  # above the group lambda_max
    print(f"{kind} {shape} {mode}: largest gap {worst:.3e}")
    assert worst <= R.MEASURED_GAP[kind], worst


def test_the_bound_follows_from_the_measurement():
    for kind in R.KINDS:
        assert R.PARITY_BOUND[kind] == 10.0 * R.MEASURED_GAP[kind] and R.PARITY_BOUND[kind] <= 1e-6


def test_the_groups_of_the_problems_cover_what_they_are_there_for():
    for kind in R.KINDS:
        for shape in R.SHAPES[kind]:
            sizes = R.sizes_for(shape[1])
            off = np.concatenate([[0], np.cumsum(sizes)])
            assert sum(sizes) == shape[1] and 1 in sizes and max(sizes) > 32
            assert any(a < 32 < b for a, b in zip(off[:-1], off[1:]))  # a group crosses a multiple of 32


# ------------------------------------------------------------------------------------------------ the plan
def _plan(ap, n, sizes):
    L, lib = ap._lib, ap._lib.load()
    sz = np.ascontiguousarray(sizes, dtype=np.int64)
    first = np.zeros(300, dtype=np.int64)
    nwg, budget = C.c_int32(0), C.c_int64(0)
    rc = lib.admm_group_multi_plan(n, sz.ctypes.data_as(C.POINTER(C.c_int64)), sz.size,
                                   first.ctypes.data_as(C.POINTER(C.c_int64)), first.size, C.byref(nwg), C.byref(budget))
    return rc, first[:nwg.value + 1], budget.value


@pytest.mark.parametrize("n,sizes", ((700, [1, 127, 1, 200, 3, 300, 68]), (33, [33]), (31, [1] * 31), (8300, [8300]),
                                     (10000, [10] * 1000), (10000, [1000] * 10), (40000, [1] * 40000),
                                     (65536, [1] * 65536), (100000, [7] * 14285 + [5])))
def test_plan_packs_whole_groups_and_covers_every_row(ap, n, sizes):
    rc, first, budget = _plan(ap, n, sizes)
    assert rc == ap._lib.E_OK if hasattr(ap._lib, "E_OK") else rc == 0
    off = np.concatenate([[0], np.cumsum(sizes)])
    assert first[0] == 0 and first[-1] == n and np.all(np.diff(first) > 0)  # 0 .. n without gaps
    assert set(first) <= set(off)                                           # whole groups only
    assert len(first) - 1 <= 256                                            # kScgMaxWg partial sums per fit
    assert budget >= 32 and budget & (budget - 1) == 0                      # one row block, doubled
    rows, groups = np.diff(first), np.diff(np.searchsorted(off, first))
    assert np.all(groups <= 256)                                            # kGmMaxGroups scales in LDS
    assert np.all((rows <= budget) | (groups == 1))                         # past the budget: a workgroup to itself


def test_plan_refusals(ap):
    L = ap._lib
    for n, sizes, code, part in ((6, [3, 0, 3], L.E_INVALID, "group 1 has a size below 1"),
                                 (6, [3, 2], L.E_INVALID, "sum to 5"),
                                 (70000, [1] * 70000, L.E_UNSUPPORTED, "more than 65536 groups")):
        rc, _, _ = _plan(ap, n, sizes)
        assert rc == code and part in L.load().admm_last_error().decode()


def test_the_new_symbols_are_exported(ap):
    L = ap._lib
    for name in ("admm_sparse_lasso_set_groups", "admm_lasso_multi_set_groups", "admm_op_group_soft_threshold_multi",
                 "admm_group_multi_plan"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(L.load(), name)
    assert ap.SparseLassoMulti.set_groups is ap.LassoMulti.set_groups
