"""The multi-fit robust regression on a sparse design matrix without a device: the NumPy restatement of
the matrix-free loop against the oracle's Cholesky loop (this also MEASURES the parity tolerance of test_gpu_sparse_reg),
and the argument checks and refusals of the Python surface and of the C ABI that fire before the device is touched."""
import ctypes as C

import numpy as np
import pytest

import sparse_reg_restated as R
from sparse_cases import Csc, csc_of, desc_of


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_restatement_matches_the_oracle_and_measures_the_parity_gap(ap, shape, mode):
    """every fit, with nodualerror 1 and 0, every field (dnorm / derr included), no entry excluded"""
    c = R.case(ap, shape, mode)
    worst = 0.0
    for nd in (1, 0):
        steps = []
        for k in range(len(R.FITS)):
            ref = R.oracle_fit(ap, shape, mode, k, nd)
            got = R.restated_fit(c, k, nd)
            assert got["steps"] == ref["steps"], (k, nd, got["steps"], ref["steps"])
            assert ("dnorm" in ref and not np.isnan(ref["dnorm"]).any()) == (nd == 0)
            gap = R.relgap(got, ref)
            print(f"{shape} {mode} nodualerror={nd} fit {k}: steps {ref['steps']}, gap {gap:.3e}, "
                  f"inner iterations {got['cg_iters_total']}")
            assert got["cg_capped_updates"] == 0
            steps.append(ref["steps"])
            worst = max(worst, gap)
        # the oracle alone stops the fits at different iterations: the test of freezing
        assert len(set(steps)) >= (5 if nd else 3), steps
        if nd == 0:  # the dual residual decides: every fit runs past its nodualerror = 1 stop, and some still stop early
            assert sum(s < R.DUAL_MAXITERS for s in steps) >= 2, steps
            assert all(s > R.oracle_fit(ap, shape, mode, k, 1)["steps"] for k, s in enumerate(steps)), steps
    print(f"{shape} {mode}: largest gap {worst:.3e}")
    assert worst <= R.MEASURED_GAP, worst


def test_restatement_on_the_tall_problem_sits_inside_the_measured_gap(ap):
    """the 8200 x 40 problem of test_gpu_sparse_reg (a workgroup takes two row blocks) belongs to the measurement"""
    c = R.tall_case(ap)
    for k in R.TALL_FITS:
        ref = R.tall_oracle(ap, k)
        got = R.restated_fit(c, k, 1, maxiters=R.TALL_MAXITERS)
        gap = R.relgap(got, ref)
        print(f"{R.TALL} fit {k}: steps {ref['steps']}, gap {gap:.3e}")
        assert got["steps"] == ref["steps"] and gap <= R.MEASURED_GAP


def test_the_bound_follows_from_the_measurement():
    assert R.PARITY_BOUND == 10.0 * R.MEASURED_GAP and R.PARITY_BOUND <= 1e-6


def test_restated_loop_on_rank_deficient_matrices(ap):
    """what the oracle cannot run: the minimum-norm x-update keeps x = 0.0 on an empty column and equal coefficients on
    a duplicated one"""
    A = R.matrix(ap, 257, 65, 0.03, full_rank=False)
    assert np.linalg.matrix_rank(A) == 64 and not A[:, 7].any()
    c = R.case(ap, (257, 65, 0.03), "shared", A=A)
    got = R.restated_fit(c, 0, 1)
    assert got["xopt"][7] == 0.0 and got["steps"] < 1000
    B = A.copy()
    B[:, 7] = B[:, 9]
    c = R.case(ap, (257, 65, 0.03), "shared", A=B)
    got = R.restated_fit(c, 1, 1)
    assert abs(got["xopt"][7] - got["xopt"][9]) <= 1e-12 * np.max(np.abs(got["xopt"]))


def _sparse_problem(ap):
    c = R.case(ap, (257, 65, 0.03), "shared")
    return c["D"], c["S"][:, 0]


@pytest.mark.parametrize("name,value", [("fast", 1), ("convtest", 1), ("relax", 1.5), ("adaptive", 1),
                                        ("xsolve", "inverse"), ("xsolve", "trsv"), ("comm", object()),
                                        ("parallel", "both"), ("stopcond", "hnorm"), ("stopcond", "both")])
def test_options_refused_by_name_without_a_device(ap, name, value):
    D, s = _sparse_problem(ap)
    fits = [dict(kind="lad"), dict(kind="huber")]
    for call in (lambda: ap.robustfit_multi(D, s, fits, {name: value}),
                 lambda: ap.quantilereg_multi(D, s, [0.1, 0.9], {name: value}),
                 lambda: ap.lad(D, s, {name: value}), lambda: ap.huberfit(D, s, {name: value}),
                 lambda: ap.quantilereg(D, s, 0.3, {name: value})):
        with pytest.raises(ValueError) as err:
            call()
        assert name in str(err.value), str(err.value)


def test_argument_checks_without_a_device(ap):
    D, s = _sparse_problem(ap)
    with pytest.raises(ValueError, match="rows"):
        ap.robustfit_multi(D, s[:-1], [dict(kind="lad")], {})
    with pytest.raises(ValueError, match="rows"):
        ap.lad(D, s[:-1], {})
    with pytest.raises(ValueError, match="fit 1"):
        ap.robustfit_multi(D, s, [dict(kind="lad"), dict(kind="lad", tau=1.5)], {})
    with pytest.raises(ValueError, match="columns"):
        ap.robustfit_multi(D, np.zeros((257, 3)), [dict(kind="lad"), dict(kind="huber")], {})
    with pytest.raises(ValueError, match="x0"):
        ap.robustfit_multi(D, s, [dict(kind="lad"), dict(kind="huber")], dict(x0=np.zeros((65, 3))))
    with pytest.raises(ValueError, match="z0"):
        ap.huberfit(D, s, dict(z0=np.zeros(5)))
    with pytest.raises(ValueError, match="x0"):
        ap.lad(D, s, dict(x0=np.zeros(5)))
    with pytest.raises(ValueError):
        ap.lad(D, s, dict(weights=-np.ones(257)))
    with pytest.raises(ValueError, match="tau"):
        ap.quantilereg(D, s, 1.0, {})
    for xs in ("auto", "cg", "CG"):  # they pass the check: the next one fires
        with pytest.raises(ValueError, match="z0"):
            ap.lad(D, s, dict(xsolve=xs, z0=np.zeros(5)))
    # the dense surface is as it was: getproxops keeps refusing a sparse D for the regression family
    for name in ("lad", "huberfit"):
        with pytest.raises(Exception):
            ap.getproxops(name, dict(D=D, s=s))


def test_abi_symbols_structs_and_defaults(ap):
    L = ap._lib
    lib = L.load()
    for name in ("desc_default", "options_default", "create", "run", "fetch", "set_weights", "chunk", "destroy"):
        assert "admm_sparse_reg_" + name in L.EXPORTED_SYMBOLS and hasattr(lib, "admm_sparse_reg_" + name)
    d = L.SparseRegDesc()
    lib.admm_sparse_reg_desc_default(C.byref(d))
    assert d.struct_size == C.sizeof(L.SparseRegDesc) and (d.K, d.ns) == (1, 1)
    o = L.SparseRegOptions()
    lib.admm_sparse_reg_options_default(C.byref(o))
    assert o.struct_size == C.sizeof(L.SparseRegOptions)
    assert (o.maxiters, o.rho, o.abstol, o.reltol, o.relax) == (1000, 1.0, 1e-5, 1e-3, 1.0)
    assert (o.cg_tol, o.cg_maxit, o.nodualerror) == (1e-12, 200, 1)
    assert ap.SparseRegMulti.chunk() == ap.SparseSvmOvr.chunk()  # the layout is shared with the sparse product
    assert lib.admm_abi_version() == 5


def raw_create(L, csc, S, K, ns=1, kind=None, a=None, delta=None, comm=None, mem=None):
    """admm_sparse_reg_create itself: (rc, handle)"""
    lib = L.load()
    sd = desc_of(L, csc, mem=mem)
    d = L.SparseRegDesc()
    lib.admm_sparse_reg_desc_default(C.byref(d))
    S = np.asfortranarray(S, dtype=np.float64)
    d.K, d.D, d.S, d.ns = K, C.pointer(sd), L.as_dp(S), ns
    keep = []
    if kind is not None:
        keep.append(np.ascontiguousarray(kind, dtype=np.int32))
        d.kind = keep[-1].ctypes.data_as(C.POINTER(C.c_int32))
    for name, v in (("a", a), ("delta", delta)):
        if v is not None:
            keep.append(np.ascontiguousarray(v, dtype=np.float64))
            setattr(d, name, L.as_dp(keep[-1]))
    if comm is not None:
        d.comm = comm
    h = C.c_void_p()
    rc = lib.admm_sparse_reg_create(C.byref(d), C.byref(h))
    return rc, h


def refusal_cases(L, c):
    """(name, expected code, message part, positional and keyword arguments of raw_create)"""
    csc = csc_of(c["D"])
    bad = Csc(csc.shape, csc.data, csc.ir, np.concatenate([[1], csc.jc[1:]]))
    S = c["S"]
    return [("jc[0] != 0", L.E_INVALID, "", (bad, S, 3), {}),
            ("D not in host arrays", L.E_INVALID, "host", (csc, S, 3), dict(mem=L.MEM_DEVICE)),
            ("K = 0", L.E_INVALID, "K >= 1", (csc, S, 0), {}),
            ("kind 2", L.E_INVALID, "fit 1", (csc, S, 3), dict(kind=[0, 2, 0])),
            ("a slope of 0", L.E_INVALID, "fit 2", (csc, S, 3), dict(a=[1.0, 1.0, 0.0])),
            ("delta on a LAD fit", L.E_INVALID, "fit 0", (csc, S, 3), dict(kind=[0, 1, 1], delta=[0.5, 0.5, 0.5])),
            ("ns = 2 for K = 3", L.E_INVALID, "columns", (csc, np.zeros((257, 2)), 3), dict(ns=2)),
            ("a communicator", L.E_UNSUPPORTED, "row-sharded", (csc, S, 3), dict(comm=C.c_void_p(1)))]


def test_abi_refusals_fire_before_the_device_is_touched(ap):
    """each of them returns its code with no handle on a machine without any device"""
    L = ap._lib
    c = R.case(ap, (257, 65, 0.03), "shared")
    for name, code, part, args, kw in refusal_cases(L, c):
        rc, h = raw_create(L, *args, **kw)
        msg = L.load().admm_last_error().decode()
        assert rc == code and not h.value and part in msg, (name, rc, msg)
