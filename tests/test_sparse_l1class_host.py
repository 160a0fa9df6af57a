"""The sparse linear classifier on a sparse design matrix without a device: the NumPy restatement of the
matrix-free loop (sparse_l1class_restated) against the optimality conditions and against the Cholesky restatement
(l1class_restated.run; this re-measures part of the parity tolerance of test_gpu_sparse_l1class), the three new structs,
and the argument checks and refusals of the Python surface and of the C ABI that fire before the device is touched."""
import ctypes as C

import numpy as np
import pytest

import l1class_restated as LR
import sparse_l1class_restated as R
from sparse_cases import Csc, csc_of, desc_of, problem
from test_l1class_host import _header, _struct_fields

SMALL = (257, 65, 0.03)


# ------------------------------------------------------------------------------------------------------------- 1. KKT
@pytest.mark.parametrize("loss", ("logistic", "sqhinge"))
def test_the_cg_restatement_satisfies_the_optimality_conditions(ap, loss):
    """test_l1class_host's bound, derived there from the stop tolerances: at the stop of a run with abstol = reltol =
    1e-10 the violation at x := z2 is at most derr + ||D||_2 * Lphi * (1 + ||D||_2) * perr.  The x-update's own residual
    (cg_tol = 1e-12 relative) enters pnorm and dnorm, which the run's stop has bounded by perr and derr."""
    p = problem(ap, 120, 30, 0.2)
    A, D = p["A"], p["D"]
    ell = np.where(A @ p["testx"] >= 0, 1.0, -1.0)
    fit = LR.Fit(loss=loss, ridge=0.05)
    fit.lam = 0.3 * LR.lambda_max(A, ell, fit)
    res = R.run(D, ell, fit, dict(abstol=1e-10, reltol=1e-10, maxiters=200000))
    assert res["steps"] < 200000 and res["cg_capped_updates"] == 0
    z2 = res["zopt"][A.shape[0]:]
    nD = np.linalg.norm(A, 2)
    lphi = fit.C * float(fit.cost(ell).max()) * (0.25 if loss == "logistic" else 2.0)
    bound = res["derr"][-1] + nD * lphi * (1.0 + nD) * res["perr"][-1]
    viol = LR.kkt(A, ell, fit, z2)
    print(f"{loss}: steps {res['steps']}, kkt violation {viol:.3e}, bound {bound:.3e}, nonzeros {np.count_nonzero(z2)}")
    assert 0 < np.count_nonzero(z2) < A.shape[1]
    assert viol <= bound


# ---------------------------------------------------------------------------------------------- 2. the parity gap
def test_the_gap_to_the_cholesky_restatement_stays_below_the_recorded_one(ap):
    """257 x 65, both label modes, both stop rules, all seven fits per iteration, and the free-running runs under
    nodualerror = 1 (the whole measurement, the 1000-iteration runs under nodualerror = 0 included, is recorded in
    sparse_l1class_restated): every field and history entry, none excluded"""
    worst = 0.0
    for mode in R.MODES:
        for nd in (0, 1):
            for k in range(R.K):
                runs = [(R.PARITY_LOOP, False)] + ([(None, True)] if nd else [])
                for loop, free in runs:
                    got = R.restated_fit(ap, SMALL, mode, k, loop, nd, free=free)
                    ref = R.cholesky_fit(ap, SMALL, mode, k, loop, nd, free=free)
                    assert got["steps"] == ref["steps"] and got["cg_capped_updates"] == 0
                    gap = R.relgap(got, ref)
                    print(f"{mode} nodualerror={nd} fit {k} free={free}: steps {ref['steps']}, gap {gap:.3e}")
                    worst = max(worst, gap)
    print(f"largest gap {worst:.3e} (recorded {R.MEASURED_GAP:g})")
    assert worst <= R.MEASURED_GAP


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_the_recorded_free_running_references(ap, shape, mode):
    """tests/golden/sparse_l1class/free_dual_*.npz hold the seven free-running runs under nodualerror = 0 of the CG
    restatement (record_free_dual).  Every file: seven runs, every field, the step counts that the GPU test asserts
    distinct; the two cheapest fits (above lambda_max, and the squared hinge) are recomputed and agree with the record
    far inside MEASURED_GAP (another machine's dot products may round differently: 1e-3 of the gap), and the recorded
    run of the fit above lambda_max lies within MEASURED_GAP of the Cholesky restatement."""
    runs = R.recorded_free_dual(shape, mode)
    m, n = R.case(ap, shape, mode)["A"].shape
    assert len(runs) == R.K and len({r["steps"] for r in runs}) >= R.FREE_DISTINCT
    for r in runs:
        assert r["xopt"].shape == (n,) and r["zopt"].shape == (m + n,) == r["uopt"].shape and r["cg_capped_updates"] == 0
        for key in ("pnorm", "perr", "dnorm", "derr", "objevals"):
            assert r[key].shape == (r["steps"],) and np.isfinite(r[key]).all()
    for k in (3, 5):
        fresh = R.restated_fit(ap, shape, mode, k, None, 0, free=True)
        assert fresh["steps"] == runs[k]["steps"]
        gap = R.relgap(fresh, runs[k])
        print(f"{shape} {mode} fit {k}: steps {fresh['steps']}, fresh against recorded {gap:.3e}")
        assert gap <= 1e-3 * R.MEASURED_GAP
    chol = R.cholesky_fit(ap, shape, mode, 3, None, 0, free=True)
    assert chol["steps"] == runs[3]["steps"] and R.relgap(runs[3], chol) <= R.MEASURED_GAP


def test_the_bound_follows_from_the_measurement():
    assert R.PARITY_BOUND == 10.0 * R.MEASURED_GAP and R.PARITY_BOUND <= 1e-6


# ---------------------------------------------------------------------------------------------- 3. structs, defaults
@pytest.mark.parametrize("cname, pyname", (("admm_sparse_l1class_desc", "SparseL1ClassDesc"),
                                           ("admm_sparse_l1class_options", "SparseL1ClassOptions"),
                                           ("admm_sparse_l1class_summary", "SparseL1ClassSummary")))
def test_structs_agree_with_the_header(ap, cname, pyname):
    L = ap._lib
    fields = _struct_fields(_header(), cname)
    st = getattr(L, pyname)
    rename = {"lambda": "lam"}
    assert [rename.get(n, n) for n, _ in fields] == [n for n, _ in st._fields_]
    for (name, ctype), (pname, ptype) in zip(fields, st._fields_):
        assert C.sizeof(ctype) == C.sizeof(ptype), (name, pname)

    class Twin(C.Structure):
        _fields_ = [(n, t) for n, t in fields]

    assert C.sizeof(Twin) == C.sizeof(st)


def test_sizes_defaults_and_symbols(ap):
    L = ap._lib
    lib = L.load()
    names = ("desc_default", "options_default", "create", "run", "fetch", "set_cost", "set_l1weights", "chunk", "destroy")
    for name in names:
        assert "admm_sparse_l1class_" + name in L.EXPORTED_SYMBOLS and hasattr(lib, "admm_sparse_l1class_" + name)
    d = L.SparseL1ClassDesc()
    lib.admm_sparse_l1class_desc_default(C.byref(d))
    assert d.struct_size == C.sizeof(L.SparseL1ClassDesc) == 96
    assert (d.K, d.nell, d.C, d.xsolve) == (1, 1, 1.0, L.XSOLVE_AUTO) and not d.loss and not d.comm
    o = L.SparseL1ClassOptions()
    lib.admm_sparse_l1class_options_default(C.byref(o))
    assert o.struct_size == C.sizeof(L.SparseL1ClassOptions) == C.sizeof(L.SparseLassoOptions) == 104
    assert (o.maxiters, o.rho, o.abstol, o.reltol, o.relax) == (1000, 1.0, 1e-5, 1e-3, 1.0)
    assert (o.cg_tol, o.cg_maxit, o.nodualerror, o.check_every) == (1e-12, 200, 0, 0)
    assert C.sizeof(L.SparseL1ClassSummary) == 40
    assert ap.SparseL1Classifier.chunk() == ap.SparseLassoMulti.chunk() == 10
    assert lib.admm_abi_version() == 5


# ---------------------------------------------------------------------------------------------- 4. Python refusals
def _data(ap):
    c = R.case(ap, SMALL, "perfit")
    return c["D"], c["ELL"][:, :2]


@pytest.mark.parametrize("name,value", [("fast", 1), ("convtest", 1), ("relax", 1.5), ("adaptive", 1),
                                        ("xsolve", "inverse"), ("xsolve", "trsv"), ("comm", object()),
                                        ("parallel", "both"), ("stopcond", "both")])
def test_options_refused_by_name_without_a_device(ap, name, value):
    D, E = _data(ap)
    for call in (lambda: ap.l1classifier_multi(D, E, [0.1, 0.2], {name: value}),
                 lambda: ap.l1classifier(D, E[:, 0], 0.1, {name: value}),
                 lambda: ap.l1classifier_path(D, E[:, 0], 4, {name: value})):
        with pytest.raises(ValueError) as err:
            call()
        assert name in str(err.value) and "on a sparse D" in str(err.value), str(err.value)


@pytest.mark.parametrize("call, message", (
    (lambda ap, D, E: ap.l1classifier(D, E[:-1, 0], 0.1), "rows in argument D"),
    (lambda ap, D, E: ap.l1classifier_multi(D, np.hstack([E, E[:, :1]]), [0.1, 0.2]), "3 columns for 2 fits"),
    (lambda ap, D, E: ap.l1classifier(D, np.where(E[:, 0] > 0, 1.0, 0.0), 0.1), r"labels \+1 and -1"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(lossfunction="01")), "0-1 loss is not convex"),
    (lambda ap, D, E: ap.l1classifier_multi(D, E, [0.1, 0.2], dict(lossfunction=["hinge", "01"])), "fit 1: lossfunction"),
    (lambda ap, D, E: ap.l1classifier_path(D, E[:, 0], 3, dict(lossfunction="01")), "0-1 loss is not convex"),
    (lambda ap, D, E: ap.l1classifier_multi(D, E, [0.1, -1.0]), "fit 1: lambda"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(l1weights=-np.ones(65))), "l1weights: every weight"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(weights=-np.ones(257))), "weights: every weight"),
    (lambda ap, D, E: ap.l1classifier_multi(D, E, [0.1, 0.2], dict(ridge=[0.1, -1.0])), "fit 1: ridge"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(C=0.0)), "options.C"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(z0=np.zeros(257))), "options.z0 does not have 322 entries"),
    (lambda ap, D, E: ap.l1classifier_multi(D, E, [0.1, 0.2], dict(u0=np.zeros((322, 1)))), "options.u0 is not a 322 x 2"),
    (lambda ap, D, E: ap.l1classifier_multi(D, E, [0.1, 0.2], dict(xsolve="cg", x0=np.zeros((64, 2)))), "options.x0"),
    (lambda ap, D, E: ap.l1classifier_path(D, E[:, 0], 0), "options.nlambda"),
))
def test_argument_errors_on_a_sparse_D(ap, call, message):
    D, E = _data(ap)
    with pytest.raises(ValueError, match=message):
        call(ap, D, E)


def test_lambda_max_on_a_sparse_D(ap):
    """The sparse D gives the dense value to m ulp of the column's absolute sum, not to the last bit: SciPy's CSC
    transposed product and the dense BLAS product add the same m terms c_i*ell_i*D_ij in different orders, and m*eps
    times the sum of their magnitudes bounds the difference of two such sums."""
    c = R.case(ap, SMALL, "shared")
    D, A, ell = c["D"], c["A"], c["ELL"][:, 0]
    m = A.shape[0]
    eps = np.finfo(np.float64).eps
    for k in (0, 4, 5, R.FAMILY):
        fit = c["fits"][k]
        o = fit.options()
        dense = ap.l1classifier_lambda_max(A, ell, o)
        sparse = ap.l1classifier_lambda_max(D, ell, o)
        absum = fit.C * LR.SLOPE0[fit.loss] * float(np.max(np.abs(A).T @ fit.cost(ell)))
        if fit.pen.w is not None:
            absum /= float(np.min(fit.pen.w[fit.pen.w > 0]))
        print(f"fit {k}: dense {dense!r} sparse {sparse!r}")
        assert abs(dense - sparse) <= m * eps * absum and dense > 0
        assert dense == pytest.approx(LR.lambda_max(A, ell, fit), rel=1e-14)


def test_the_synthetic_problem_and_the_path_grid_inputs(ap):
    import scipy.sparse as sp
    p = ap.synth.sparse_design_classifier_problem(3, 400, 80, 0.1)
    D, ell, x = p["D"], p["ell"], p["testx"]
    assert sp.issparse(D) and D.shape == (400, 80) and D.format == "csc" and D.has_canonical_format
    nrm = np.sqrt(np.asarray(D.multiply(D).sum(axis=0))).reshape(-1)
    assert np.allclose(nrm[nrm > 0], 1.0)
    assert set(np.unique(ell)) == {-1.0, 1.0} and 0 < np.count_nonzero(x) <= 24
    hit = (D @ x) != 0.0  # (a row whose nonzeros miss every active coefficient has the score 0: its label is noise)
    assert hit.sum() > 100 and np.mean(np.where((D @ x)[hit] >= 0, 1.0, -1.0) == ell[hit]) > 0.8


# ---------------------------------------------------------------------------------------------- 5. the C ABI
def raw_create(L, csc, ELL, lams, nell=None, loss=None, ridge=None, nonneg=None, l1weights=None, comm=None, mem=None,
               K=None, xsolve=None, Cv=None):
    """admm_sparse_l1class_create itself: (rc, handle)"""
    lib = L.load()
    sd = desc_of(L, csc, mem=mem)
    d = L.SparseL1ClassDesc()
    lib.admm_sparse_l1class_desc_default(C.byref(d))
    ELL = np.asfortranarray(ELL, dtype=np.float64)
    ELL = ELL.reshape(-1, 1) if ELL.ndim == 1 else ELL
    lam = np.ascontiguousarray(lams, dtype=np.float64)
    d.K, d.D, d.ELL, d.lam = (lam.size if K is None else K), C.pointer(sd), L.as_dp(ELL), L.as_dp(lam)
    d.nell = ELL.shape[1] if nell is None else nell
    keep = []
    for name, v in (("ridge", ridge), ("l1weights", l1weights)):
        if v is not None:
            keep.append(np.ascontiguousarray(v, dtype=np.float64))
            setattr(d, name, L.as_dp(keep[-1]))
    for name, v in (("nonneg", nonneg), ("loss", loss)):
        if v is not None:
            keep.append(np.ascontiguousarray(v, dtype=np.int32))
            setattr(d, name, keep[-1].ctypes.data_as(C.POINTER(C.c_int32)))
    if comm is not None:
        d.comm = comm
    if xsolve is not None:
        d.xsolve = xsolve
    if Cv is not None:
        d.C = Cv
    h = C.c_void_p()
    rc = lib.admm_sparse_l1class_create(C.byref(d), C.byref(h))
    return rc, h


def refusal_cases(L, c):
    """(name, expected code, message part, positional and keyword arguments of raw_create)"""
    csc = csc_of(c["D"])
    bad = Csc(csc.shape, csc.data, csc.ir, np.concatenate([[1], csc.jc[1:]]))
    E = c["ELL"][:, :3]
    E0 = E.copy(order="F")
    E0[5, 1] = 0.0
    lam = [0.1, 0.2, 0.3]
    w = np.ones(csc.shape[1])
    return [("jc[0] != 0", L.E_INVALID, "", (bad, E, lam), {}),
            ("D not in host arrays", L.E_INVALID, "host", (csc, E, lam), dict(mem=L.MEM_DEVICE)),
            ("K = 0", L.E_INVALID, "K >= 1", (csc, E, lam), dict(K=0)),
            ("nell = 2 for K = 3", L.E_INVALID, "2 columns", (csc, E[:, :2], lam), {}),
            ("a label of 0", L.E_INVALID, "label 5 of column 1", (csc, E0, lam), {}),
            ("the 0-1 loss", L.E_INVALID, "fit 1: the 0-1 loss", (csc, E, lam),
             dict(loss=[L.LOSS_HINGE, L.LOSS_01, L.LOSS_LOGISTIC])),
            ("an unknown loss", L.E_INVALID, "fit 2: unknown loss", (csc, E, lam),
             dict(loss=[L.LOSS_HINGE, L.LOSS_SQHINGE, 4])),
            ("a negative lambda", L.E_INVALID, "fit 1: lambda", (csc, E, [0.1, -0.2, 0.3]), {}),
            ("an infinite ridge", L.E_INVALID, "fit 0: ridge", (csc, E, lam), dict(ridge=[np.inf, 0.0, 0.0])),
            ("nonneg 2", L.E_INVALID, "fit 1: nonneg", (csc, E, lam), dict(nonneg=[0, 2, 0])),
            ("a negative weight", L.E_INVALID, "weight 4", (csc, E, lam),
             dict(l1weights=np.where(np.arange(w.size) == 4, -1.0, w))),
            ("a NaN weight", L.E_INVALID, "weight 9", (csc, E, lam),
             dict(l1weights=np.where(np.arange(w.size) == 9, np.nan, w))),
            ("C = 0", L.E_INVALID, "desc.C", (csc, E, lam), dict(Cv=0.0)),
            ("xsolve = inverse", L.E_UNSUPPORTED, "xsolve", (csc, E, lam), dict(xsolve=L.XSOLVE_INVERSE)),
            ("a communicator", L.E_UNSUPPORTED, "row-sharded", (csc, E, lam), dict(comm=C.c_void_p(1)))]


def test_abi_refusals_fire_before_the_device_is_touched(ap):
    """each of them returns its code with no handle on a machine without any device"""
    L = ap._lib
    c = R.case(ap, SMALL, "perfit")
    for name, code, part, args, kw in refusal_cases(L, c):
        rc, h = raw_create(L, *args, **kw)
        msg = L.load().admm_last_error().decode()
        assert rc == code and not h.value and msg and part in msg, (name, rc, msg)
