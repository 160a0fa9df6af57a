"""The linear SVM on a sparse design matrix on the device: the multi-vector sparse product against an
exactly summed reference and against admm_op_spmv bit for bit, the K lock-step runs against the oracle per class, the
0-1 loss under its margin guard, two chunks, costs, linearsvm(<sparse>), the reported iteration cap, reruns, refusals.

Parity bound.  The sparse lasso's 1e-7 is not copied: its operator carries +rho*I and this one does not.  The largest
relative gap between the NumPy restatement (cg_tol = 1e-13) and the oracle over these exact problems and fields is
7.26e-11, measured by test_sparse_svm_host (hinge on 600x120); the bound here is 10x the recorded 7.3e-11 = 7.3e-10 --
the factor covers the device's summation order inside the products -- and below the project's 1e-6 parity definition.
The oracle has no logistic or squared-hinge loss: those classes are compared against the oracle's unwrappedadmm (dense
pinv) with the restated prox (svm_cost_restated.run), as test_gpu_svm_cost does."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import sparse_svm_restated as R
import svm_cost_restated as SC
from sparse_cases import csc_of, desc_of
from sparse_cases import problem as lasso_problem
from test_sparse_svm_host import PARITY_BOUND, raw_create, refusal_cases

pytestmark = pytest.mark.gpu

HIST = ("pnorm", "perr", "Hnormsq", "objevals")


# ------------------------------------------------------------------------------------------------ 1. the product
def _op_matrices(ap):
    """the matrices of test_gpu_sparse's operator test, built the same way"""
    rng = np.random.default_rng(11)
    dense = lambda r, c, d: np.where(rng.random((r, c)) < d, rng.standard_normal((r, c)), 0.0)
    tiny = np.zeros((5, 3))  # row 1 and column 1 empty
    tiny[[0, 2], 0] = [1.5, -2.0]
    tiny[[3, 4], 2] = [0.25, 3.0]
    long_row = dense(200, 300, 0.01)  # one row of n nonzeros among short ones
    long_row[17, :] = rng.standard_normal(300)
    prob = lambda r, c, d: lasso_problem(ap, r, c, d, seed=r + c)["A"]
    return {
        "1x1": np.array([[-1.75]]),
        "5x3 empty row and column": tiny,
        "257x65 3%": prob(257, 65, 0.03),
        "600x120 5%": prob(600, 120, 0.05),
        "80x200 10%": prob(80, 200, 0.10),
        "130x300 50%": dense(130, 300, 0.5),   # rows of ~150: 64 lanes walk them with a remainder
        "64x64 5%": dense(64, 64, 0.05),       # ~3 per row: the sub-wave groups
        "40x300 4%": dense(40, 300, 0.04),     # ~12 per row: 16 lanes
        "200x300 1% with a full row": long_row,
        "7x9 all zero": np.zeros((7, 9)),
    }


@pytest.fixture(scope="module")
def op_matrices(ap):
    return _op_matrices(ap)


def _spmm(L, csc, transpose, X):
    rows, cols = csc.shape
    Y = np.full((cols if transpose else rows, X.shape[1]), np.nan, order="F")
    d = desc_of(L, csc)
    L.check(L.load().admm_op_spmm(C.byref(d), int(transpose), X.shape[1], L.as_dp(X), L.as_dp(Y)))
    return Y


def _spmv(L, csc, transpose, x):
    rows, cols = csc.shape
    y = np.full(cols if transpose else rows, np.nan)
    d = desc_of(L, csc)
    L.check(L.load().admm_op_spmv(C.byref(d), int(transpose), L.as_dp(np.ascontiguousarray(x)), L.as_dp(y)))
    return y


def _exact_rows(A, x):
    """per row: the exactly rounded sum of the exact products, the sum of their magnitudes, the number of nonzeros"""
    ref, mag, k = np.zeros(A.shape[0]), np.zeros(A.shape[0]), np.zeros(A.shape[0], dtype=np.int64)
    fx = [Fraction(float(v)) for v in x]
    for i in range(A.shape[0]):
        nz = np.nonzero(A[i])[0]
        terms = [Fraction(float(A[i, j])) * fx[j] for j in nz]
        ref[i] = float(sum(terms, Fraction(0)))
        mag[i] = float(sum((abs(t) for t in terms), Fraction(0)))
        k[i] = nz.size
    return ref, mag, k


@pytest.mark.parametrize("name", ["1x1", "5x3 empty row and column", "257x65 3%", "600x120 5%", "80x200 10%",
                                  "130x300 50%", "64x64 5%", "40x300 4%", "200x300 1% with a full row", "7x9 all zero"])
@pytest.mark.parametrize("transpose", [0, 1])
def test_spmm_against_an_exactly_summed_reference_and_spmv_bits(gpu, op_matrices, name, transpose):
    """per entry |y - ref| <= 2 k 2^-53 sum|a||x| (the bound of test_gpu_sparse's product test); an empty row is +0.0;
    column c has the bits of admm_op_spmv on column c; a second call returns the same bits -- for K in 1, 3, Kc, Kc + 1"""
    L = gpu._lib
    A = op_matrices[name]
    M = A.T if transpose else A
    kc = gpu.SparseSvmOvr.chunk()
    Xall = np.asfortranarray(np.random.default_rng(5).standard_normal((M.shape[1], kc + 1)))
    csc = csc_of(sp.csc_matrix(A))
    exact = [_exact_rows(M, Xall[:, c]) for c in range(kc + 1)]
    single = [_spmv(L, csc, transpose, Xall[:, c]) for c in range(kc + 1)]
    for K in sorted({1, 3, kc, kc + 1}):
        X = np.asfortranarray(Xall[:, :K])
        Y = _spmm(L, csc, transpose, X)
        assert not np.isnan(Y).any()
        for c in range(K):
            ref, mag, k = exact[c]
            bound = 2.0 * k * 2.0 ** -53 * mag
            assert float(np.max(np.abs(Y[:, c] - ref) - bound)) <= 0.0, (name, K, c)
            assert np.all(Y[k == 0, c] == 0.0) and not np.signbit(Y[k == 0, c]).any()
            assert np.array_equal(Y[:, c], single[c]), (name, K, c)
        assert np.array_equal(Y, _spmm(L, csc, transpose, X))


# ------------------------------------------------------------------------------------------------ the runs
def _close(name, got, ref, tol):
    got, ref = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(ref, dtype=np.float64))
    assert got.shape == ref.shape, f"{name}: shape {got.shape} vs {ref.shape}"
    assert not np.isnan(got).any() and not np.isnan(ref).any(), f"{name}: NaN"
    if ref.ndim == 1 and not name.split("[")[0].endswith("opt"):
        scale = np.maximum(np.abs(ref), 1e-12 + 1e-3 * np.max(np.abs(ref)))  # scalar histories: per entry
        err = float(np.max(np.abs(got - ref) / scale))
    else:
        err = float(np.max(np.abs(got - ref)) / max(1e-300, np.max(np.abs(ref))))
    print(f"{name}: relative error {err:.3e} (bound {tol:g})")
    assert err < tol, f"{name}: relative error {err:.3e} >= {tol:g}"


def _compare_class(got, c, ref, tol, keys=HIST, limit=None):
    """column c of a one-vs-rest result against one oracle run, over the class's own steps (or the first `limit`)"""
    if limit is None:
        assert int(got["steps"][c]) == ref["steps"], (c, got["steps"][c], ref["steps"])
    k = int(got["steps"][c]) if limit is None else limit
    for key in keys:
        if key in ref:
            _close(f"{key}[{c}]", got[key][:k, c], np.asarray(ref[key])[:k], tol)
    if limit is None:
        assert np.isnan(got["pnorm"][k:, c]).all()  # NaN past the class's last step
        for key in ("xopt", "zopt", "uopt"):
            _close(f"{key}[{c}]", got[key][:, c], ref[key], tol)
        _close(f"objopt[{c}]", [got["objopt"][c]], [ref["objopt"]], tol)


def _options(p, cols=None, **more):
    cols = list(range(p["x0"].shape[1])) if cols is None else list(cols)
    return dict(objevals=1, cg_tol=1e-13, x0=np.asfortranarray(p["x0"][:, cols]), z0=np.asfortranarray(p["z0"][:, cols]),
                u0=np.asfortranarray(p["u0"][:, cols]), **more)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_three_losses_match_the_oracle_per_class(gpu, shape):
    p = R.problem(gpu, *shape)
    refs = [R.oracle_class(gpu, shape, c, loss) for c, loss in enumerate(R.LOSSES3)]
    assert len({r["steps"] for r in refs}) == 3  # the classes stop at different iterations: the test of freezing
    got = gpu.linearsvm_ovr(p["D"], p["labels"], p["C"], _options(p, classes=np.arange(3.0), lossfunction=list(R.LOSSES3)))
    assert got["xsolve"] == "cg" and got["nnz"] == p["D"].nnz
    assert list(got["steps"]) == [r["steps"] for r in refs]
    assert got["pnorm"].shape == (max(r["steps"] for r in refs), 3)
    for c in range(3):
        _compare_class(got, c, refs[c], PARITY_BOUND)
    assert np.array_equal(got["cg_capped_updates"], np.zeros(3, dtype=np.int64))
    assert np.all(got["cg_iters_total"] >= got["steps"])
    assert np.all(got["xopt"][7, :] == 0.0)  # the empty column: exactly 0.0


def test_01_loss_margin_guarded(gpu):
    """the 0-1 prox is discontinuous (q24): compared over the first k iterations, where no component of the oracle's own
    run sits within 1e-6 of a decision boundary of minz01 (getProxOps.m:1175), as test_gpu_svm_ovr guards it"""
    shape = (257, 65, 0.03)
    p = R.problem(gpu, *shape)
    ell, Cc, A = p["ELL"][:, 0], p["C"], p["A"]
    ref = R.oracle_class(gpu, shape, 0, "01")
    k, u = 0, p["u0"][:, 0]
    for i in range(min(ref["steps"], 40)):
        sarg = ell * (A @ ref["xvals"][:, i] + u)
        margin = min(np.min(np.abs(sarg - 1.0)), np.min(np.abs(sarg - (1 - np.sqrt(2.0 * Cc)))))
        if margin < 1e-6:
            break
        u = ref["uvals"][:, i]
        k = i + 1
    assert k >= 10, k  # (the seed was chosen on the CPU: the guard cannot silently skip the comparison)
    got = gpu.linearsvm_ovr(p["D"], p["labels"], Cc, _options(p, [0], classes=[0.0], lossfunction="01"))
    assert got["steps"][0] >= k
    _compare_class(got, 0, ref, PARITY_BOUND, keys=("pnorm", "perr", "objevals"), limit=k)


def test_two_chunks(gpu):
    """K = Kc + 1: the lone class of the second chunk and class 0 each equal their oracle run"""
    shape = (257, 65, 0.03)
    p = R.problem(gpu, *shape)
    kc = gpu.SparseSvmOvr.chunk()
    cols = [c % 3 for c in range(kc + 1)]
    losses = [R.LOSSES3[c] for c in cols]
    got = gpu.linearsvm_ovr(p["D"], p["labels"], p["C"], _options(p, cols, classes=np.array(cols, dtype=np.float64),
                                                                  lossfunction=losses))
    assert got["xopt"].shape == (65, kc + 1)
    for c in (0, kc):
        _compare_class(got, c, R.oracle_class(gpu, shape, cols[c], losses[c]), PARITY_BOUND)
    for c in range(3, kc + 1):  # a class gets the same bits wherever it lands
        for key in ("xopt", "zopt", "uopt", "pnorm", "objevals"):
            assert np.array_equal(got[key][:, c], got[key][:, c - 3], equal_nan=True), (key, c)


def test_weights_and_balanced_class_costs(gpu):
    shape = (257, 65, 0.03)
    p = R.problem(gpu, *shape)
    w = np.random.default_rng(21).uniform(0.25, 4.0, 257)
    w[::17] = 0.0
    losses = ["hinge", "sqhinge"]
    got = gpu.linearsvm_ovr(p["D"], p["labels"], p["C"], _options(p, [0, 1], classes=[0.0, 1.0], lossfunction=losses,
                                                                  weights=w, classcost="balanced"))
    for c in range(2):
        ell = p["ELL"][:, c]
        ref = SC.run(p["A"], ell, p["C"], SC.cost_vector(ell, w, "balanced"), losses[c],
                     dict(objevals=1, x0=p["x0"][:, c], z0=p["z0"][:, c], u0=p["u0"][:, c]))
        _compare_class(got, c, ref, PARITY_BOUND)
    assert not got["cg_capped_updates"].any()


def test_linearsvm_on_a_sparse_matrix_is_the_one_class_object(gpu):
    p = R.problem(gpu, 257, 65, 0.03)
    for c, loss in ((1, "logistic"), (2, "hinge")):
        o = dict(objevals=1, cg_tol=1e-13, lossfunction=loss)
        one = gpu.linearsvm(p["D"], p["ELL"][:, c], p["C"], dict(o, x0=p["x0"][:, c], z0=p["z0"][:, c], u0=p["u0"][:, c]))
        ovr = gpu.linearsvm_ovr(p["D"], p["labels"], p["C"], dict(_options(p, [c], classes=[float(c)]), lossfunction=loss))
        assert one["steps"] == int(ovr["steps"][0]) and one["xsolve"] == "cg" and one["nnz"] == p["D"].nnz
        assert "xvals" not in one and one["xopt"].shape == (65,)
        for key in ("xopt", "zopt", "uopt") + HIST:
            assert np.array_equal(one[key], ovr[key][:, 0]), key
        assert one["objopt"] == ovr["objopt"][0] and one["cg_iters_total"] == int(ovr["cg_iters_total"][0])
        assert one["cg_capped_updates"] == 0


def test_the_iteration_cap_is_reported(gpu):
    p = R.problem(gpu, 600, 120, 0.05)
    got = gpu.linearsvm_ovr(p["D"], p["labels"], p["C"], dict(_options(p, classes=np.arange(3.0),
                                                                       lossfunction=list(R.LOSSES3)), cg_tol=1e-13,
                                                              cg_maxit=2))
    assert np.all(got["steps"] >= 1) and np.isfinite(got["xopt"]).all()
    assert np.all(got["cg_capped_updates"] > 0)
    assert np.all(got["cg_iters_total"] <= 2 * got["steps"])


def test_rerun_and_check_every_give_the_same_bits(gpu):
    L = gpu._lib
    p = R.problem(gpu, 257, 65, 0.03)
    obj = gpu.SparseSvmOvr(p["D"], p["ELL"], p["C"], list(R.LOSSES3))
    try:
        runs = []
        for ce in (0, 0, 1, 7):
            summ = obj.run(objevals=1, check_every=ce, cg_tol=1e-13, z0=p["z0"], u0=p["u0"])
            S = int(summ["steps"].max())
            runs.append([summ["steps"], summ["objopt"], summ["cg_iters_total"], summ["cg_capped_updates"]] +
                        [obj.fetch(f, r) for f, r in ((L.OVR_F_XOPT, 65), (L.OVR_F_ZOPT, 257), (L.OVR_F_UOPT, 257),
                                                      (L.OVR_F_PNORM, S), (L.OVR_F_PERR, S), (L.OVR_F_HNORMSQ, S),
                                                      (L.OVR_F_OBJEVALS, S))])
    finally:
        obj.close()
    assert len(set(runs[0][0])) == 3
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.size > 0 and np.array_equal(a, b, equal_nan=True)


def test_refusals_through_the_c_abi(gpu):
    """each returns its code with no handle, and a well-formed create succeeds right behind it"""
    L = gpu._lib
    p = R.problem(gpu, 257, 65, 0.03)
    csc = csc_of(p["D"])
    for name, code, args in refusal_cases(L, p):
        rc, h = raw_create(L, *args)
        assert rc == code and not h.value, (name, rc, L.load().admm_last_error())
        rc, h = raw_create(L, csc, p["ELL"], 3)
        assert rc == L.OK and h.value, (name, L.load().admm_last_error())
        L.load().admm_sparse_svm_destroy(h)
