"""The host side of the sparse lasso, no GPU: the binding layer's checks of a sparse args.D, the
conversion of scipy.sparse inputs to canonical CSC, and the sparse problem generator."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from sparse_cases import Csc


@pytest.fixture(scope="module")
def B(ap):
    ap._lib.load()
    from admm_project_amd import binding
    return binding


# 5 x 3:  column 0 = rows {0, 2}, column 1 = empty, column 2 = rows {1, 3, 4}
GOOD = dict(shape=(5, 3), data=[1.0, 2.0, 3.0, 4.0, 5.0], ir=[0, 2, 1, 3, 4], jc=[0, 2, 2, 5])


def _args(csc, s=None):
    args = dict(D=csc, s=np.arange(1.0, 6.0) if s is None else s, rho=1.0)
    args["lambda"] = 0.1
    return args


def _bad(**change):
    return Csc(**dict(GOOD, **change))


@pytest.mark.parametrize("name,csc,s", [
    ("jc does not start at 0", _bad(jc=[1, 2, 2, 5]), None),
    ("decreasing jc", _bad(jc=[0, 2, 1, 5]), None),
    ("jc[cols] != nnz", _bad(jc=[0, 2, 2, 4]), None),
    ("row index == rows", _bad(ir=[0, 2, 1, 3, 5]), None),
    ("unsorted rows in a column", _bad(ir=[0, 2, 3, 1, 4]), None),
    ("duplicate entry", _bad(ir=[0, 2, 1, 1, 4]), None),
    ("NaN value", _bad(data=[1.0, 2.0, float("nan"), 4.0, 5.0]), None),
    ("s of the wrong length", Csc(**GOOD), np.ones(4)),
])
def test_binding_refuses_a_malformed_sparse_matrix(ap, B, name, csc, s):
    with pytest.raises(ap._lib.AdmmError) as err:
        B.Binding("lasso", _args(csc, s))
    assert err.value.code == ap._lib.E_INVALID, (name, str(err.value))


def test_binding_messages_name_the_first_offending_column(ap, B):
    for csc, col in ((_bad(ir=[0, 2, 1, 3, 5]), 2), (_bad(ir=[2, 0, 1, 3, 4]), 0), (_bad(jc=[0, 2, 1, 5]), 1)):
        with pytest.raises(ap._lib.AdmmError) as err:
            B.Binding("lasso", _args(csc))
        assert f"column {col}" in str(err.value), str(err.value)


def test_binding_describes_a_well_formed_sparse_matrix(ap, B):
    b = B.Binding("lasso", _args(Csc(**GOOD)))
    assert b.sparse() == dict(rows=5, cols=3, nnz=5)
    d = b.desc
    assert (d.problem, d.m, d.n) == (ap._lib.PROB_LASSO, 5, 3) and not d.D
    assert b.info()["nA"] == 3
    dense = B.Binding("lasso", _args(np.ones((5, 3))))
    assert dense.sparse() is None


def test_binding_refuses_sparse_data_for_other_problems(ap, B):
    for problem in ("lad", "huberfit", "linearsvm"):
        with pytest.raises(ap._lib.AdmmError) as err:
            B.Binding(problem, dict(D=Csc(**GOOD), s=np.ones(5), ell=np.ones(5), C=1.0))
        assert err.value.code == ap._lib.E_UNSUPPORTED and problem in str(err.value)
    for extra in (dict(parallel=1, slices=[2, 3]), dict(L=np.eye(3))):
        with pytest.raises(ap._lib.AdmmError) as err:
            B.Binding("lasso", dict(_args(Csc(**GOOD)), **extra))
        assert err.value.code == ap._lib.E_UNSUPPORTED


def _arrays(d):
    nnz, cols = int(d.nnz), int(d.cols)
    return (np.ctypeslib.as_array(d.val, (max(nnz, 1),))[:nnz].copy(),
            np.ctypeslib.as_array(d.ir, (max(nnz, 1),))[:nnz].astype(np.int64),
            np.ctypeslib.as_array(d.jc, (cols + 1,)).astype(np.int64))


def test_scipy_inputs_reach_the_ctypes_layer_as_canonical_csc(ap):
    L = ap._lib
    rng = np.random.default_rng(3)
    A = np.where(rng.random((9, 6)) < 0.4, rng.standard_normal((9, 6)), 0.0)
    r, c = np.nonzero(A)
    order = rng.permutation(r.size)
    # COO with unsorted indices and every entry split into two duplicates
    coo = sp.coo_matrix((np.concatenate([0.25 * A[r, c][order], 0.75 * A[r, c][order]]),
                         (np.concatenate([r[order], r[order]]), np.concatenate([c[order], c[order]]))), shape=A.shape)
    for M in (coo, sp.csr_matrix(A), sp.csc_matrix(A), sp.csr_array(A)):
        keep = []
        d = L.sparse_desc(M, keep)
        val, ir, jc = _arrays(d)
        assert (d.rows, d.cols, d.nnz, d.mem) == (9, 6, np.count_nonzero(A), L.MEM_HOST)
        assert jc[0] == 0 and jc[-1] == d.nnz and np.all(np.diff(jc) >= 0)
        for j in range(6):
            assert np.all(np.diff(ir[jc[j]:jc[j + 1]]) > 0)  # ascending, no duplicates
        back = sp.csc_matrix((val, ir, jc), shape=(9, 6)).toarray()
        np.testing.assert_allclose(back, M.toarray(), rtol=0, atol=1e-15)
        np.testing.assert_allclose(back, A, rtol=0, atol=1e-15)
    assert not L.is_sparse(A) and not L.is_sparse(None) and L.is_sparse(coo)


def test_sparse_lasso_problem_is_deterministic_with_unit_columns(ap):
    p, q = (ap.synth.sparse_lasso_problem(5, 300, 40, 0.05) for _ in range(2))
    assert sp.issparse(p["D"]) and p["D"].format == "csc" and p["D"].shape == (300, 40)
    assert p["D"].has_canonical_format
    assert np.array_equal(p["D"].toarray(), q["D"].toarray()) and np.array_equal(p["s"], q["s"]) and p["lam"] == q["lam"]
    other = ap.synth.sparse_lasso_problem(6, 300, 40, 0.05)
    assert not np.array_equal(other["D"].toarray(), p["D"].toarray())
    A = p["D"].toarray()
    nrm = np.sqrt(np.sum(A * A, axis=0))
    assert np.all((np.abs(nrm - 1.0) < 1e-12) | (nrm == 0.0)) and np.count_nonzero(nrm) >= 35
    assert 0.03 < p["D"].nnz / A.size < 0.07
    assert p["lam"] == pytest.approx(0.1 * np.max(np.abs(A.T @ p["s"])))
    empty = ap.synth.sparse_lasso_problem(0, 7, 9, 0.0)
    assert empty["D"].nnz == 0 and empty["D"].shape == (7, 9)
