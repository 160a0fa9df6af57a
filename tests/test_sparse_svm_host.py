"""The linear SVM on a sparse design matrix without a device: the NumPy restatement of the matrix-free
loop against the oracle's pinv loop (this also MEASURES the parity tolerance of test_gpu_sparse_svm), the argument
checks and refusals of the Python surface and of the C ABI that fire before the device is touched, and the CSC
canonicalisation."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import sparse_svm_restated as R
from sparse_cases import Csc, csc_of, desc_of

# the largest relative gap between the restatement (cg_tol = 1e-13) and the oracle over SHAPES x LOSSES3 x FIELDS, as
# test_restatement_matches_the_oracle_and_measures_the_parity_gap printed it (hinge on 600x120: 7.26e-11)
MEASURED_GAP = 7.3e-11
PARITY_BOUND = 10.0 * MEASURED_GAP  # the device's bound: the factor covers its summation order inside the products
assert PARITY_BOUND <= 1e-6  # never looser than the project's parity definition


@pytest.mark.parametrize("shape", R.SHAPES)
def test_restatement_matches_the_oracle_and_measures_the_parity_gap(ap, shape):
    p = R.problem(ap, *shape)
    steps, worst = [], 0.0
    for c, loss in enumerate(R.LOSSES3):
        ref = R.oracle_class(ap, shape, c, loss)
        got = R.run(p["A"], p["ELL"][:, c], p["C"], loss,
                    dict(objevals=1, x0=p["x0"][:, c], z0=p["z0"][:, c], u0=p["u0"][:, c]), cg_tol=1e-13)
        assert got["steps"] == ref["steps"], (loss, got["steps"], ref["steps"])
        gap = R.relgap(got, ref)
        print(f"{shape} {loss}: steps {ref['steps']}, gap {gap:.3e}, inner iterations {got['cg_iters_total']}")
        assert got["cg_capped_updates"] == 0
        assert got["xopt"][7] == 0.0  # the empty column: CG from 0 never leaves range(D')
        steps.append(ref["steps"])
        worst = max(worst, gap)
    assert len(set(steps)) == 3, steps  # the oracle alone stops the three classes at different iterations
    assert worst <= MEASURED_GAP, worst


def test_restated_cg_edge_cases():
    rng = np.random.default_rng(0)
    D = rng.standard_normal((9, 4))
    D[:, 2] = 0.0
    xm = R.CgPinv(D, 1e-13, 50)
    z = rng.standard_normal(9)
    x = xm(None, z, np.zeros(9), 1.0)
    assert x[2] == 0.0 and np.allclose(x, np.linalg.pinv(D) @ z, atol=1e-12)
    assert np.array_equal(xm(None, np.zeros(9), np.zeros(9), 1.0), np.zeros(4))  # zero right-hand side: x = 0, no division
    capped = R.CgPinv(D, 1e-13, 1)
    capped(None, z, np.zeros(9), 1.0)
    assert capped.capped == 1 and capped.total == 1


def _sparse_problem(ap):
    p = R.problem(ap, 257, 65, 0.03)
    return p["D"], p["labels"], p["ELL"][:, 0], p["C"]


@pytest.mark.parametrize("name,value", [("fast", 1), ("convtest", 1), ("relax", 1.5), ("adaptive", 1),
                                        ("xsolve", "inverse"), ("xsolve", "trsv"), ("Dplus", np.zeros((65, 257))),
                                        ("comm", object()), ("parallel", "both")])
def test_options_refused_by_name_without_a_device(ap, name, value):
    D, labels, ell, Cc = _sparse_problem(ap)
    for call in (lambda: ap.linearsvm_ovr(D, labels, Cc, {name: value}), lambda: ap.linearsvm(D, ell, Cc, {name: value})):
        with pytest.raises(ValueError) as err:
            call()
        assert name in str(err.value), str(err.value)


def test_argument_checks_without_a_device(ap):
    D, labels, ell, Cc = _sparse_problem(ap)
    with pytest.raises(ValueError, match="sizes incompatible"):
        ap.linearsvm_ovr(D, labels[:-1], Cc, {})
    with pytest.raises(ValueError, match="sizes incompatible"):
        ap.linearsvm(D, ell[:-1], Cc, {})
    with pytest.raises(ValueError, match="nonnegative"):
        ap.linearsvm_ovr(D, labels, -1.0, {})
    with pytest.raises(ValueError, match="x0"):
        ap.linearsvm_ovr(D, labels, Cc, dict(x0=np.zeros((65, 2))))
    with pytest.raises(ValueError, match="z0"):
        ap.linearsvm(D, ell, Cc, dict(z0=np.zeros(5)))
    with pytest.raises(ValueError, match="lossfunction"):
        ap.linearsvm_ovr(D, labels, Cc, dict(lossfunction=["hinge"]))
    with pytest.raises(ValueError, match="weights"):
        ap.linearsvm_ovr(D, labels, Cc, dict(weights=-np.ones(257)))
    with pytest.raises(ValueError, match="auto"):  # xsolve = 'auto' and 'cg' pass the check: the next one fires
        ap.linearsvm_ovr(D, labels, Cc, dict(xsolve="pinv"))
    for xs in ("auto", "cg", "CG"):
        with pytest.raises(ValueError, match="z0"):
            ap.linearsvm(D, ell, Cc, dict(xsolve=xs, z0=np.zeros(5)))
    # the dense surface is as it was: getproxops keeps refusing a sparse D for the SVM
    with pytest.raises(Exception):
        ap.getproxops("LinearSVM", dict(D=D, ell=ell, C=Cc, lossfunction="hinge"))


def test_csc_canonicalisation(ap):
    L = ap._lib
    rows, cols = np.array([4, 0, 2, 0, 4, 1]), np.array([1, 1, 0, 1, 1, 2])
    vals = np.array([1.0, 2.0, 3.0, 0.5, -4.0, 7.0])  # (0, 1) and (4, 1) twice, rows of column 1 out of order
    M = sp.coo_matrix((vals, (rows, cols)), shape=(5, 3))
    r, c, val, ir, jc = L.canonical_csc(M)
    assert (r, c) == (5, 3) and ir.dtype == np.uint64 and jc.dtype == np.uint64 and val.dtype == np.float64
    assert list(jc) == [0, 1, 3, 4] and list(ir) == [2, 0, 4, 1] and list(val) == [3.0, 2.5, -3.0, 7.0]
    assert M.nnz == 6  # the caller's matrix is not reordered in place
    for other in (M.tocsr(), sp.csc_array(M), sp.lil_matrix(M.toarray())):
        assert all(np.array_equal(a, b) for a, b in zip(L.canonical_csc(other)[2:], (val, ir, jc)))
    with pytest.raises(TypeError):
        L.canonical_csc(M.toarray())


def test_abi_symbols_structs_and_defaults(ap):
    L = ap._lib
    lib = L.load()
    for name in ("admm_op_spmm", "admm_op_spmm_cg", "admm_sparse_svm_desc_default", "admm_sparse_svm_options_default",
                 "admm_sparse_svm_create", "admm_sparse_svm_run", "admm_sparse_svm_fetch", "admm_sparse_svm_set_cost",
                 "admm_sparse_svm_chunk", "admm_sparse_svm_destroy"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    d = L.SparseSvmDesc()
    lib.admm_sparse_svm_desc_default(C.byref(d))
    assert d.struct_size == C.sizeof(L.SparseSvmDesc) and d.K == 1
    o = L.SparseSvmOptions()
    lib.admm_sparse_svm_options_default(C.byref(o))
    assert o.struct_size == C.sizeof(L.SparseSvmOptions)
    assert (o.maxiters, o.rho, o.abstol, o.reltol, o.Hnormtol, o.relax) == (1000, 1.0, 1e-5, 1e-3, 1e-6, 1.0)
    assert (o.cg_tol, o.cg_maxit) == (1e-12, 200)  # the engine's xsolve = 'cg' defaults
    kc = ap.SparseSvmOvr.chunk()
    assert 2 <= kc <= 10 and kc % 2 == 0
    assert lib.admm_abi_version() == 5


def raw_create(L, csc, ELL, K, loss=None, comm=None):
    """admm_sparse_svm_create itself: (rc, handle)"""
    lib = L.load()
    sd = desc_of(L, csc)
    d = L.SparseSvmDesc()
    lib.admm_sparse_svm_desc_default(C.byref(d))
    ELL = np.asfortranarray(ELL, dtype=np.float64)
    d.K, d.D, d.ELL, d.C = K, C.pointer(sd), L.as_dp(ELL), 1.0
    lossv = None
    if loss is not None:
        lossv = np.ascontiguousarray(loss, dtype=np.int32)
        d.loss = lossv.ctypes.data_as(C.POINTER(C.c_int32))
    if comm is not None:
        d.comm = comm
    h = C.c_void_p()
    rc = lib.admm_sparse_svm_create(C.byref(d), C.byref(h))
    return rc, h


def refusal_cases(L, p):
    """(name, expected code, arguments of raw_create): malformed jc, labels of 0.5, K = 0, loss code 9, a communicator"""
    csc = csc_of(p["D"])
    bad = Csc(csc.shape, csc.data, csc.ir, np.concatenate([[1], csc.jc[1:]]))
    half = p["ELL"].copy()
    half[11, 1] = 0.5
    return [("jc[0] != 0", L.E_INVALID, (bad, p["ELL"], 3)),
            ("a label of 0.5", L.E_INVALID, (csc, half, 3)),
            ("K = 0", L.E_INVALID, (csc, p["ELL"], 0)),
            ("loss code 9", L.E_INVALID, (csc, p["ELL"], 3, [0, 9, 0])),
            ("a communicator", L.E_UNSUPPORTED, (csc, p["ELL"], 3, None, C.c_void_p(1)))]


def test_abi_refusals_fire_before_the_device_is_touched(ap):
    """each of them returns its code with no handle on a machine without any device"""
    L = ap._lib
    p = R.problem(ap, 257, 65, 0.03)
    for name, code, args in refusal_cases(L, p):
        rc, h = raw_create(L, *args)
        assert rc == code and not h.value, (name, rc, L.load().admm_last_error())
    d = desc_of(L, csc_of(p["D"]))
    x = np.zeros((65, 2), order="F")
    y = np.zeros((257, 2), order="F")
    assert L.load().admm_op_spmm(C.byref(d), 0, 0, L.as_dp(x), L.as_dp(y)) == L.E_INVALID  # K = 0
    # admm_op_spmm_cg (every refusal: test_spmm_cg_host): K = 0, tol = 0, and D with jc[0] != 0
    state = np.zeros((2, 6), dtype=np.int64)
    sp_ = state.ctypes.data_as(C.POINTER(C.c_int64))
    cg = lambda dd, K, tol: L.load().admm_op_spmm_cg(C.byref(dd), K, L.as_dp(x), None, 1.0, tol, 10, 0, None, L.as_dp(x),
                                                     None, sp_, None)
    assert cg(d, 0, 1e-10) == L.E_INVALID and cg(d, 2, 0.0) == L.E_INVALID
    assert cg(desc_of(L, refusal_cases(L, p)[0][2][0]), 2, 1e-10) == L.E_INVALID
