"""The lasso on a sparse design matrix on the device: the sparse matrix-vector product against an
exactly summed reference, the sparse engine against the oracle's factor path on the dense array, the penalty family over
sparse data against its restatements, the refusals, and device-resident CSC arrays."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import grouplasso_restated as G
import penalty_restated as P
from oracle import solvers_ref as S
from sparse_cases import Csc, csc_of, desc_of, problem
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

_CACHE = {}


def _problem(ap, rows, cols, density):
    key = (rows, cols, density)
    if key not in _CACHE:
        _CACHE[key] = problem(ap, rows, cols, density, seed=rows + cols)
    return _CACHE[key]


def _spmv(L, csc, transpose, x):
    rows, cols = csc.shape
    y = np.full(cols if transpose else rows, np.nan)
    d = desc_of(L, csc)
    L.check(L.load().admm_op_spmv(C.byref(d), int(transpose), L.as_dp(x), L.as_dp(y)))
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


def _op_matrices(ap):
    rng = np.random.default_rng(11)
    dense = lambda r, c, d: np.where(rng.random((r, c)) < d, rng.standard_normal((r, c)), 0.0)
    tiny = np.zeros((5, 3))  # row 1 and column 1 empty
    tiny[[0, 2], 0] = [1.5, -2.0]
    tiny[[3, 4], 2] = [0.25, 3.0]
    long_row = dense(200, 300, 0.01)  # one row of n nonzeros among short ones
    long_row[17, :] = rng.standard_normal(300)
    return {
        "1x1": np.array([[-1.75]]),
        "5x3 empty row and column": tiny,
        "257x65 3%": _problem(ap, 257, 65, 0.03)["A"],
        "600x120 5%": _problem(ap, 600, 120, 0.05)["A"],
        "80x200 10%": _problem(ap, 80, 200, 0.10)["A"],
        "130x300 50%": dense(130, 300, 0.5),   # rows of ~150: 64 lanes walk them with a remainder
        "64x64 5%": dense(64, 64, 0.05),       # ~3 per row: the sub-wave groups
        "40x300 4%": dense(40, 300, 0.04),     # ~12 per row: 16 lanes
        "200x300 1% with a full row": long_row,
        "7x9 all zero": np.zeros((7, 9)),
    }


@pytest.mark.parametrize("name", ["1x1", "5x3 empty row and column", "257x65 3%", "600x120 5%", "80x200 10%",
                                  "130x300 50%", "64x64 5%", "40x300 4%", "200x300 1% with a full row", "7x9 all zero"])
@pytest.mark.parametrize("transpose", [0, 1])
def test_spmv_against_an_exactly_summed_reference(gpu, name, transpose):
    """|y_i - ref_i| <= 2 k_i 2^-53 sum_j |a_ij||x_j|: the bound of a k-term fp64 sum in any order, doubled for the
    reference's own final rounding; an empty row is exactly 0.0; a second call returns the same bits"""
    L = gpu._lib
    A = _op_matrices(gpu)[name]
    M = A.T if transpose else A
    x = np.random.default_rng(5).standard_normal(M.shape[1])
    csc = csc_of(sp.csc_matrix(A))
    y = _spmv(L, csc, transpose, x)
    ref, mag, k = _exact_rows(M, x)
    bound = 2.0 * k * 2.0 ** -53 * mag
    worst = float(np.max(np.abs(y - ref) - bound))
    print(f"{name} transpose={transpose}: max |y - ref| = {np.max(np.abs(y - ref)):.3e}, max bound = {np.max(bound):.3e}")
    assert not np.isnan(y).any()
    assert worst <= 0.0, (name, worst)
    assert np.all(y[k == 0] == 0.0) and not np.signbit(y[k == 0]).any()
    assert np.array_equal(y, _spmv(L, csc, transpose, x))


def test_spmv_and_spmm_non_temporal_forms_are_exact_on_integers(gpu):
    """spmv_plan streams (non-temporal index and value loads, spmv_kernel / spmm_kernel <., true>) once both stored
    orientations pass kStreamBytes: 24 nnz + 8 (rows + cols + 2) > 192 MiB, from 8.4 million nonzeros.  30001 x 4001
    with one entry in 14 (8.57 million; rows of ~286 and ~2143 nonzeros: 64 lanes, odd remainders), nonzero integers in
    [-4, 4] against integers in [-8, 8]: every partial sum is an integer below 2^53, so both products are compared bit
    for bit with SciPy's, in both orientations; the multi-vector product (K = 3) column by column."""
    L = gpu._lib
    rows, cols = 30001, 4001
    rng = np.random.default_rng(31)
    keep = rng.integers(0, 14, size=(cols, rows), dtype=np.int8) == 0
    vals = rng.integers(1, 5, size=(cols, rows), dtype=np.int8) * (2 * rng.integers(0, 2, size=(cols, rows), dtype=np.int8) - 1)
    A = sp.csr_matrix(np.where(keep, vals, 0).astype(np.int8)).T.astype(np.float64)  # CSR of A' = CSC of A
    csc = csc_of(A)
    nnz = csc.data.size
    assert 24 * nnz + 8 * (rows + cols + 2) > 192 << 20 and csc.shape == (rows, cols)
    for transpose in (0, 1):
        M = A.T.tocsr() if transpose else A.tocsr()
        X = np.asfortranarray(rng.integers(-8, 9, size=(M.shape[1], 3)).astype(np.float64))
        ref = M @ X
        assert np.all(ref == np.rint(ref)) and np.max(np.abs(ref)) < 2.0 ** 40
        y = _spmv(L, csc, transpose, np.ascontiguousarray(X[:, 0]))
        assert np.array_equal(y, ref[:, 0]), (transpose, np.flatnonzero(y != ref[:, 0])[:8])
        Y = np.full(ref.shape, np.nan, order="F")
        L.check(L.load().admm_op_spmm(C.byref(desc_of(L, csc)), transpose, 3, L.as_dp(X), L.as_dp(Y)))
        assert np.array_equal(Y, ref), (transpose, np.argwhere(Y != ref)[:8])


def _check_sparse_run(got, D):
    assert got["cg_capped_updates"] == 0
    assert got["xsolve"] == "cg" and got["nnz"] == D.nnz
    assert got["engine_info"]["xsolve_used"] == "cg" and got["engine_info"]["factor_n"] == 0


@pytest.mark.parametrize("shape,opts", [
    ((600, 120, 0.05), dict()),
    ((600, 120, 0.05), dict(rho=3.0, relax=1.5)),
    ((600, 120, 0.05), dict(fast=1, fasttype="strong", maxiters=40)),
    ((80, 200, 0.10), dict()),  # fat: the oracle takes lasso.m:172's branch, the engine the same CG
])
def test_sparse_lasso_matches_the_factor_path_on_the_dense_array(gpu, shape, opts):
    p = _problem(gpu, *shape)
    o = dict(objevals=1, quiet=1, **opts)
    got = gpu.lasso(p["D"], p["s"], p["lam"], dict(o, cg_tol=1e-13))
    ref = S.lasso(p["A"], p["s"], p["lam"], o)
    _compare(got, ref, tol=1e-7)
    _check_sparse_run(got, p["D"])


@pytest.mark.parametrize("kind", ["grouplasso", "elasticnet", "nonnegative weighted"])
def test_penalty_family_over_sparse_data(gpu, kind):
    p = _problem(gpu, 257, 65, 0.03)
    o = dict(objevals=1, quiet=1)
    if kind == "grouplasso":
        sizes = [5] * 13
        got = gpu.grouplasso(p["D"], p["s"], p["lam"], sizes, dict(o, cg_tol=1e-13))
        ref = G.run(p["A"], p["s"], p["lam"], sizes, o)
    elif kind == "elasticnet":
        got = gpu.elasticnet(p["D"], p["s"], p["lam"], 0.5, dict(o, cg_tol=1e-13))
        ref = P.run(p["A"], p["s"], p["lam"], P.Penalty(ridge=0.5), o)
    else:
        pen = P.Penalty(l1weights=np.random.default_rng(9).uniform(0.25, 2.0, 65), nonnegative=1)
        got = gpu.lasso(p["D"], p["s"], p["lam"], dict(o, cg_tol=1e-13, **pen.options()))
        ref = P.run(p["A"], p["s"], p["lam"], pen, o)
    _compare(got, ref, tol=1e-7)
    _check_sparse_run(got, p["D"])


def _raw_create(L, p, sd, **fields):
    """admm_engine_create_sparse itself: (rc, handle, desc)"""
    lib = L.load()
    d = L.ProblemDesc()
    lib.admm_problem_desc_default(C.byref(d))
    d.problem = L.PROB_LASSO
    d.m, d.n = p["A"].shape
    d.s = L.as_dp(p["s"])
    d.lambda_ = p["lam"]
    d.rho = 1.0
    d.mem = L.MEM_HOST
    for k, v in fields.items():
        setattr(d, k, v)
    h = C.c_void_p()
    rc = lib.admm_engine_create_sparse(C.byref(d), C.byref(sd), C.byref(h))
    return rc, h, d


def _engine_of(ap, h, d):
    eng = ap.engine.Engine.__new__(ap.engine.Engine)
    eng._lib, eng._comm = ap._lib.load(), None
    eng._attach(h, d)
    eng.sparse = True
    return eng


def test_refusals_leave_the_process_able_to_create(gpu):
    L = gpu._lib
    p = _problem(gpu, 257, 65, 0.03)
    D, s, lam = p["D"], p["s"], p["lam"]

    def refused(code, fn):
        with pytest.raises(L.AdmmError) as err:
            fn()
        assert err.value.code == code, str(err.value)
        ok = gpu.lasso(D, s, lam, dict(maxiters=3, quiet=1))  # a well-formed create right behind the refusal
        assert ok["nnz"] == D.nnz

    for xs in ("trsv", "inverse"):
        refused(L.E_UNSUPPORTED, lambda: gpu.lasso(D, s, lam, dict(xsolve=xs, quiet=1)))
    args = dict(D=D, s=s, rho=1.0)
    args["lambda"] = lam
    refused(L.E_UNSUPPORTED, lambda: gpu.api.getproxops("lasso", dict(args, L=np.eye(65))))
    refused(L.E_UNSUPPORTED, lambda: gpu.api.getproxops("lasso", dict(args, parallel=1, slices=[128, 129])))
    refused(L.E_UNSUPPORTED, lambda: gpu.lasso(D, s, lam, dict(parallel="both", workers=2, quiet=1)))

    csc = csc_of(D)

    def raw(code, sd, **fields):
        rc, h, _ = _raw_create(L, p, sd, **fields)
        assert rc == code and not h.value, (rc, L.load().admm_last_error())
        rc, h, d = _raw_create(L, p, desc_of(L, csc))
        assert rc == L.OK and h.value
        _engine_of(gpu, h, d).close()

    raw(L.E_INVALID, desc_of(L, csc), D=L.as_dp(p["A"]), ldD=257)       # desc->D given
    raw(L.E_INVALID, desc_of(L, csc), m=256)                             # desc->m != rows
    bad = Csc(csc.shape, csc.data, csc.ir, np.concatenate([[1], csc.jc[1:]]))
    raw(L.E_INVALID, desc_of(L, bad))                                    # jc[0] != 0 straight to the ABI
    raw(L.E_UNSUPPORTED, desc_of(L, csc), problem=L.PROB_LAD)
    raw(L.E_UNSUPPORTED, desc_of(L, csc), xsolve=L.XSOLVE_PINV)
    with pytest.raises(L.AdmmError) as err:                              # a dense engine has no sparse field
        gpu.engine.Engine(L.PROB_LASSO, D=p["A"], s=s, lam=lam).fetch(L.F_SPARSE_NNZ, 3)
    assert err.value.code == L.E_INVALID


def test_device_resident_csc_arrays_give_the_same_iterates(gpu):
    import torch

    L = gpu._lib
    p = _problem(gpu, 257, 65, 0.03)
    csc = csc_of(p["D"])
    dev = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda() for a in (csc.data, csc.ir, csc.jc)]
    torch.cuda.synchronize()
    runs = []
    for sd in (desc_of(L, csc), desc_of(L, csc, mem=L.MEM_DEVICE, pointers=[t.data_ptr() for t in dev])):
        rc, h, d = _raw_create(L, p, sd)
        assert rc == L.OK, L.load().admm_last_error()
        eng = _engine_of(gpu, h, d)
        summ = eng.run(maxiters=15, domaxiters=1, objevals=1)
        runs.append([eng.fetch(f, 65 * summ.steps) for f in (L.F_XVALS, L.F_ZVALS, L.F_UVALS)] +
                    [eng.fetch(L.F_OBJEVALS, summ.steps), eng.fetch(L.F_SPARSE_NNZ, 3)])
        eng.close()
    assert runs[0][4][0] == p["D"].nnz
    for a, b in zip(*runs):
        assert a.size > 0 and np.array_equal(a, b)
