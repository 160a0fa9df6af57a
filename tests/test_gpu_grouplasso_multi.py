"""Group lasso and sparse-group lasso, K fits over one D, on the device: grouplasso_multi on the dense and
the sparse object against penalty_restated.run per fit in both modes and under both stop rules, K = 12 over two chunks
against the same fits run alone (bits), set_groups between runs of one object, the reduction to the single-fit
grouplasso, the path and its tester, and the refusals through the raw C ABI and through Python.

Parity bound.  The largest relative gap between the NumPy restatement of each object's x-update (explicit inverse; CG at
cg_tol = 1e-12) and penalty_restated.run (Cholesky solves) over these exact problems, fits, both stop rules and every
field, measured by test_grouplasso_multi_host, is 9.925e-12 (dense, the 1.25*lambda_max fit on 600x257, per-fit S) and
8.925e-10 (sparse, the weighted fit on 257x65, per-fit S); the bounds here are 10x the recorded 1.0e-11 and 9.0e-10 -- the
factor q37 - q40 use for the device's summation order inside the products -- and far below the project's 1e-6.  The l1
weights are shared by all fits of an object, so every problem runs twice, all seven fits each time: without weights (fits
0 .. 5 are compared) and with them (fit 6 is)."""
import ctypes as C

import numpy as np
import pytest

import group_multi_restated as R
from test_gpu_sparse_lasso import _close

pytestmark = pytest.mark.gpu

HIST = ("pnorm", "perr", "objevals")
KEYS = ("xopt", "zopt", "uopt", "pnorm", "perr", "dnorm", "derr", "objevals")
CASES = [(kind, shape) for kind in R.KINDS for shape in R.SHAPES[kind]]


def _compare_fit(got, c, ref, dual, bound):
    """column c of a multi-fit result against one reference run: steps, every history over the fit's own steps, NaN
    beyond them, the three vectors and objopt"""
    assert int(got["steps"][c]) == ref["steps"], (c, got["steps"][c], ref["steps"])
    k = ref["steps"]
    for key in HIST + (("dnorm", "derr") if dual else ()):
        _close(f"{key}[{c}]", got[key][:k, c], np.asarray(ref[key])[:k], bound)
        assert np.isnan(got[key][k:, c]).all()  # NaN past the fit's last step
    for key in ("xopt", "zopt", "uopt"):
        _close(f"{key}[{c}]", got[key][:, c], ref[key], bound)
    _close(f"objopt[{c}]", [got["objopt"][c]], [ref["objopt"]], bound)


def _design(c, kind):
    return c["A"] if kind == "dense" else c["D"]


def _options(c, nodualerror, cols, weighted, **more):
    o = dict(objevals=1, nodualerror=nodualerror, rho=R.RHO, z0=np.asfortranarray(c["z0"][:, cols]),
             u0=np.asfortranarray(c["u0"][:, cols]), ridge=[R.RIDGE[k] for k in cols],
             nonnegative=[R.NONNEG[k] for k in cols], groupweights=c["gw"], l1=c["l1"][cols])
    if weighted:
        o["l1weights"] = c["w"]
    o.update(more)
    return o


def _multi(gpu, kind, c, nodualerror, cols=None, weighted=False, **more):
    cols = list(range(R.K)) if cols is None else list(cols)
    S = c["S"] if c["S"].shape[1] == 1 else np.asfortranarray(c["S"][:, cols])
    return gpu.grouplasso_multi(_design(c, kind), S, c["lams"][cols], c["sizes"], _options(c, nodualerror, cols, weighted, **more))


# ---------------------------------------------------------------------------------------------- 1. parity per fit
@pytest.mark.parametrize("nodualerror", (0, 1))
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("kind,shape", CASES)
def test_fits_match_the_reference_per_fit(gpu, kind, shape, mode, nodualerror):
    c = R.case(gpu, kind, shape, mode)
    dual = not nodualerror
    refs = [R.reference_fit(gpu, kind, shape, mode, k, nodualerror) for k in range(R.K)]
    assert len({r["steps"] for r in refs}) >= 5  # the fits stop at different iterations: the test of freezing
    got = _multi(gpu, kind, c, nodualerror)
    assert np.array_equal(got["groups"], c["sizes"]) and np.array_equal(got["lams"], c["lams"])
    assert ("dnorm" in got) == dual and ("nnz" in got) == (kind == "sparse")
    for k in R.PLAIN:
        _compare_fit(got, k, refs[k], dual, R.PARITY_BOUND[kind])
    assert np.all(got["zopt"][:, 4] == 0.0)  # lambda above the group lambda_max
    weighted = _multi(gpu, kind, c, nodualerror, weighted=True)
    _compare_fit(weighted, R.FAMILY, refs[R.FAMILY], dual, R.PARITY_BOUND[kind])
    assert np.all(weighted["zopt"][:, R.FAMILY] >= 0.0)
    for k in (0, 1, 2, 3, 4):  # l1_k = 0: tau_k*w_i = 0, the l1 weights do not reach these fits
        for key in KEYS:
            if key in got:
                assert np.array_equal(got[key][:, k], weighted[key][:, k], equal_nan=True), (k, key)


# ---------------------------------------------------------------------------------------------- 2. placement in bits
@pytest.mark.parametrize("kind,shape", (("dense", (300, 130)), ("sparse", (600, 120, 0.05))))
def test_twelve_fits_equal_the_same_fits_run_alone_in_bits(gpu, kind, shape):
    """K = 12 over two chunks with fits that stop at different iterations in both chunks: every fit has the bits of the
    same fit run alone, K = 1 -- neither its chunk, its column nor its stopped neighbours reach its sums"""
    c = R.case(gpu, kind, shape, "shared")
    n = c["A"].shape[1]
    frac = np.array([0.05, 0.7, 0.1, 1.25, 0.15, 0.5, 0.25, 0.9, 0.35, 0.08, 0.06, 0.6])
    lams = float(c["glmax"][0]) * frac
    l1 = float(c["lmax"][0]) * np.where(np.arange(12) % 3 == 2, 0.05, 0.0)
    rng = np.random.default_rng(5)
    z0, u0 = (np.asfortranarray(0.1 * rng.standard_normal((n, 12))) for _ in range(2))
    o = dict(objevals=1, rho=R.RHO, groupweights=c["gw"], l1weights=c["w"])
    got = gpu.grouplasso_multi(_design(c, kind), c["S"], lams, c["sizes"], dict(o, z0=z0, u0=u0, l1=l1))
    steps = [int(s) for s in got["steps"]]
    print("steps", steps)
    assert len(set(steps[:10])) >= 5 and steps[10] != steps[11] and max(steps) < 1000
    for k in range(12):
        one = gpu.grouplasso_multi(_design(c, kind), c["S"], lams[k:k + 1], c["sizes"],
                                   dict(o, z0=np.asfortranarray(z0[:, k:k + 1]), u0=np.asfortranarray(u0[:, k:k + 1]),
                                        l1=l1[k:k + 1]))
        assert int(one["steps"][0]) == steps[k]
        for key in KEYS:
            a, b = got[key][:, k], one[key][:, 0]
            if key not in ("xopt", "zopt", "uopt"):
                assert np.isnan(a[steps[k]:]).all()
                a = a[:steps[k]]
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)), (k, key)
        assert got["objopt"][k] == one["objopt"][0]


# ---------------------------------------------------------------------------------------------- 3. set_groups
def _object(gpu, kind, c):
    cols = list(range(R.K))
    args = (c["S"], c["lams"], [R.RIDGE[k] for k in cols], [R.NONNEG[k] for k in cols])
    if kind == "dense":
        return gpu.LassoMulti(c["A"], *args, rho=R.RHO)
    return gpu.SparseLassoMulti(c["D"], *args)


@pytest.mark.parametrize("kind,shape", (("dense", (200, 64)), ("sparse", (257, 65, 0.03))))
def test_set_groups_between_runs_of_one_object(gpu, kind, shape):
    c = R.case(gpu, kind, shape, "shared")
    obj = _object(gpu, kind, c)
    try:
        run = dict(objevals=1, z0=c["z0"], u0=c["u0"])
        plain = obj.results(obj.run(**run))
        obj.set_groups(c["sizes"], c["gw"], c["l1"])
        grouped = obj.results(obj.run(**run))
        obj.set_groups(c["sizes"])  # other groups' parameters: weights 1, l1 = 0
        unit = obj.results(obj.run(**run))
        with pytest.raises(gpu.AdmmError, match="weight 2"):
            obj.set_groups(c["sizes"], np.where(np.arange(c["sizes"].size) == 2, -1.0, 1.0))
        refused = obj.results(obj.run(**run))  # a refused call changes nothing
        obj.set_groups(None)
        again = obj.results(obj.run(**run))
    finally:
        obj.close()
    for k in R.PLAIN:
        _compare_fit(grouped, k, R.reference_fit(gpu, kind, shape, "shared", k, 0), True, R.PARITY_BOUND[kind])
    assert not np.array_equal(unit["zopt"], grouped["zopt"])
    for key in KEYS:
        assert np.array_equal(refused[key], unit[key], equal_nan=True), key
        assert np.array_equal(again[key], plain[key], equal_nan=True), key  # today's ungrouped results in bits
    # the ungrouped run is lasso_multi's own: the same numbers through the public caller
    caller = (gpu.lasso_multi_dense if kind == "dense" else gpu.lasso_multi)(
        _design(c, kind), c["S"], c["lams"], dict(objevals=1, rho=R.RHO, z0=c["z0"], u0=c["u0"], ridge=list(R.RIDGE),
                                                  nonnegative=list(R.NONNEG)))
    for key in KEYS:
        assert np.array_equal(caller[key], plain[key], equal_nan=True), key


# ---------------------------------------------------------------------------------------------- 4. K = 1
@pytest.mark.parametrize("kind,shape", (("dense", (200, 64)), ("sparse", (257, 65, 0.03))))
def test_one_fit_agrees_with_the_single_fit_grouplasso(gpu, kind, shape):
    c = R.case(gpu, kind, shape, "shared")
    k = 5  # the sparse-group fit
    lam, s = float(c["lams"][k]), c["S"][:, 0]
    common = dict(objevals=1, rho=R.RHO, groupweights=c["gw"], l1=float(c["l1"][k]))
    got = gpu.grouplasso_multi(_design(c, kind), s, [lam], c["sizes"],
                               dict(common, z0=np.asfortranarray(c["z0"][:, k:k + 1]), u0=np.asfortranarray(c["u0"][:, k:k + 1])))
    one = gpu.grouplasso(_design(c, kind), s, lam, c["sizes"], dict(common, z0=c["z0"][:, k], u0=c["u0"][:, k]))
    assert int(got["steps"][0]) == one["steps"]
    for key in ("xopt", "zopt", "uopt"):
        _close(key, got[key][:, 0], one[key], R.PARITY_BOUND[kind])
    for key in ("pnorm", "perr", "dnorm", "derr", "objevals"):
        _close(key, got[key][:, 0], np.asarray(one[key])[:one["steps"]], R.PARITY_BOUND[kind])


# ---------------------------------------------------------------------------------------------- 5. the path
@pytest.mark.parametrize("kind,shape", (("dense", (600, 257)), ("sparse", (600, 120, 0.05))))
def test_path_from_lambda_max_down(gpu, kind, shape):
    c = R.case(gpu, kind, shape, "shared")
    got = gpu.grouplasso_path(_design(c, kind), c["S"][:, 0], c["sizes"], None, dict(nlambda=12, groupweights=c["gw"]))
    lams = got["lams"]
    assert lams.shape == (12,) and lams[0] == c["glmax"][0] and np.all(np.diff(lams) < 0)
    dfg = [int(v) for v in got["df_groups"]]
    print("df_groups", dfg, "df", [int(v) for v in got["df"]])
    assert all(b >= a for a, b in zip(dfg[:-1], dfg[1:]))  # non-increasing in lambda
    assert dfg[0] == 0 and np.all(got["zopt"][:, 0] == 0.0) and dfg[-1] > 0
    assert np.array_equal(got["groups"], c["sizes"]) and got["df"][-1] >= dfg[-1]
    with pytest.raises(ValueError, match="give lams"):
        gpu.grouplasso_path(_design(c, kind), c["S"][:, 0], c["sizes"], None, dict(l1=0.1))


def test_the_tester_passes(gpu):
    test = gpu.testers.grouplassopathtest(seed=0)
    assert test["failed"] == 0 and test["zero_above_lmax"] and test["groups_grow"] and test["groups_enter_whole"]
    assert test["df_groups"][-1] > 0


# ---------------------------------------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("kind", R.KINDS)
def test_refusals_through_the_c_abi_and_through_python(gpu, kind):
    shape = R.SHAPES[kind][0]  # 130 and 120 coefficients: eleven groups
    c = R.case(gpu, kind, shape, "shared")
    L, lib = gpu._lib, gpu._lib.load()
    n = c["A"].shape[1]
    obj = _object(gpu, kind, c)
    fn = getattr(lib, obj._abi + "_set_groups")
    ip, dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)), L.as_dp
    sizes, G = c["sizes"], int(c["sizes"].size)
    ones = np.ones(G)
    try:
        obj.set_groups(sizes, c["gw"], c["l1"])
        before = obj.results(obj.run(objevals=1))
        zero = sizes.copy()
        zero[3], zero[4] = 0, sizes[3] + sizes[4]
        short = sizes.copy()
        short[-1] -= 1
        bad_w, nan_w = np.where(np.arange(G) == 2, -1.0, ones), np.where(np.arange(G) == 5, np.nan, ones)
        bad_l1, inf_l1 = np.where(np.arange(R.K) == 4, -0.5, 0.0), np.where(np.arange(R.K) == 6, np.inf, 0.0)
        for args, part in (((G, ip(zero), None, None), "group 3 has a size below 1"),
                           ((G, ip(short), None, None), f"not to n = {n}"),
                           ((G, ip(sizes), dp(bad_w), None), "weight 2 is negative or not finite"),
                           ((G, ip(sizes), dp(nan_w), None), "weight 5 is negative or not finite"),
                           ((G, ip(sizes), None, dp(bad_l1)), "fit 4: l1 is negative or not finite"),
                           ((G, ip(sizes), None, dp(inf_l1)), "fit 6: l1 is negative or not finite")):
            assert fn(obj._h, *args) == L.E_INVALID
            assert part in lib.admm_last_error().decode(), (part, lib.admm_last_error().decode())
        for kw, part in ((dict(groups=zero), "group 3"), (dict(groups=short), "sum to"),
                         (dict(groups=sizes, groupweights=bad_w), "weight 2"), (dict(groups=sizes, l1=bad_l1), "fit 4")):
            with pytest.raises(gpu.AdmmError, match=part):
                obj.set_groups(**kw)
        with pytest.raises(ValueError, match="integer"):  # never truncated to [.., 1, ..]
            obj.set_groups(np.where(np.arange(G) == 1, sizes - 0.5, sizes + 0.0))
        after = obj.results(obj.run(objevals=1))  # refused calls changed nothing
        for key in KEYS:
            assert np.array_equal(after[key], before[key], equal_nan=True), key
    finally:
        obj.close()
    D, S = _design(c, kind), c["S"]
    for groups, o, part in ((zero, {}, "every size must be >= 1"), (short, {}, "sizes sum to"),
                            (sizes, dict(groupweights=bad_w), "groupweights"), (sizes, dict(l1=bad_l1), "fit 4")):
        with pytest.raises(ValueError, match=part):
            gpu.grouplasso_multi(D, S, c["lams"], groups, o)


def test_a_fat_dense_matrix_is_refused_as_before(gpu):
    c = R.case(gpu, "dense", (200, 64), "shared")
    with pytest.raises(ValueError, match="stays with lasso"):
        gpu.grouplasso_multi(np.asfortranarray(c["A"][:40]), c["S"][:40], [0.1], c["sizes"], {})
    with pytest.raises(ValueError, match="stays with lasso"):
        gpu.lasso_multi_dense(np.asfortranarray(c["A"][:40]), c["S"][:40], [0.1], {})
