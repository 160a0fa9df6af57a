"""The sparse linear classifier on the host: the restated run (l1class_restated) satisfies the optimality
conditions, lambda_max is the threshold of the all-zero model, the header's structs and constants agree with _lib.py,
and the three Python functions refuse bad arguments before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import l1class_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (120, 30)


# ------------------------------------------------------------------------------------------------------------- 1. KKT
@pytest.mark.parametrize("loss", ("logistic", "sqhinge"))
def test_the_restated_run_satisfies_the_optimality_conditions(loss):
    """At the stop of a run with abstol = reltol = 1e-10 the z-update gives rho*u in the subdifferential of g at z, and
    the x-update gives rho*A'u = -rho*A'(z - zprev), whose norm is dnorm < derr.  So D'grad L(z1) + q = delta with q in
    the penalty's subdifferential at z2 and ||delta|| < derr.  kkt is evaluated at x := z2 (the iterate with exact
    zeros), where the loss's gradient is taken at D*z2 instead of z1: z1 - D*z2 = (z1 - D*x) + D*(x - z2), both parts
    bounded by pnorm < perr, and grad L is Lipschitz with Lphi = C*max(c)*max phi'' (1/4 logistic, 2 sqhinge).  Hence
        violation <= derr + ||D||_2 * Lphi * (1 + ||D||_2) * perr
    with perr and derr the run's last tolerances."""
    p = R.problem(SHAPE)
    D, ell = p["D"], p["ELL"][:, 0]
    fit = R.Fit(loss=loss, ridge=0.05)
    fit.lam = 0.3 * R.lambda_max(D, ell, fit)
    res = R.run(D, ell, fit, dict(abstol=1e-10, reltol=1e-10, maxiters=200000))
    assert res["steps"] < 200000
    m = D.shape[0]
    z2 = res["zopt"][m:]
    nD = np.linalg.norm(D, 2)
    lphi = fit.C * float(fit.cost(ell).max()) * (0.25 if loss == "logistic" else 2.0)
    bound = res["derr"][-1] + nD * lphi * (1.0 + nD) * res["perr"][-1]
    viol = R.kkt(D, ell, fit, z2)
    print(f"{loss}: steps {res['steps']}, kkt violation {viol:.3e}, bound {bound:.3e}, nonzeros {np.count_nonzero(z2)}")
    assert 0 < np.count_nonzero(z2) < D.shape[1]
    assert viol <= bound


def test_kkt_notices_a_wrong_point():
    p = R.problem(SHAPE)
    D, ell = p["D"], p["ELL"][:, 0]
    fit = R.Fit(loss="logistic")
    fit.lam = 0.3 * R.lambda_max(D, ell, fit)
    assert R.kkt(D, ell, fit, np.zeros(D.shape[1])) > 0.1 * fit.lam  # x = 0 is not optimal below lambda_max
    x = np.zeros(D.shape[1])
    x[0] = -1.0
    assert R.kkt(D, ell, R.Fit(loss="logistic", lam=fit.lam, nonnegative=1), x) == np.inf


# ------------------------------------------------------------------------------------------------------ 2. lambda_max
@pytest.mark.parametrize("loss", ("logistic", "hinge", "sqhinge"))
def test_lambda_max_is_the_threshold_of_the_zero_model(loss):
    """At lambda = lambda_max itself the critical coordinate sits ON the soft threshold (|rho*u2_j| = lambda*w_j at the
    optimum), so whether an iterate a finite run stops at has an exact zero there is a matter of rounding and of the
    stop tolerance; the factors above it are 1.01 and 1.25."""
    p = R.problem(SHAPE)
    D, ell = p["D"], p["ELL"][:, 0]
    m = D.shape[0]
    fit = R.Fit(loss=loss, weights=np.linspace(0.5, 1.5, m), classcost=(2.0, 0.5),
                l1weights=np.linspace(0.5, 2.0, D.shape[1]))
    lmax = R.lambda_max(D, ell, fit)
    for factor in (1.01, 1.25):
        fit.lam = factor * lmax
        res = R.run(D, ell, fit, dict(abstol=1e-9, reltol=1e-9, maxiters=20000))
        assert res["steps"] < 20000
        assert np.all(res["zopt"][m:] == 0.0), (loss, factor)
    fit.lam = 0.99 * lmax
    res = R.run(D, ell, fit, dict(abstol=1e-9, reltol=1e-9, maxiters=200000))
    assert np.count_nonzero(res["zopt"][m:]) > 0


# ------------------------------------------------------------------------------------------------- 3. the header, _lib
def _header():
    with open(os.path.join(ROOT, "include", "admm_engine.h")) as fh:
        return fh.read()


_CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}


def _struct_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        mt = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.+)$", decl)
        ctype, pointer, names = mt.group(2), mt.group(3), mt.group(4)
        for nm in names.split(","):
            nm = nm.strip()
            ptr = pointer or ("*" if nm.startswith("*") else "")
            out.append((nm.lstrip("* "), C.c_void_p if ptr else _CTYPE[ctype]))
    return out


@pytest.mark.parametrize("cname, pyname", (("admm_l1class_desc", "L1ClassDesc"), ("admm_l1class_options", "L1ClassOptions"),
                                           ("admm_l1class_summary", "L1ClassSummary")))
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


def test_constants_and_symbols_agree_with_the_header(ap):
    L = ap._lib
    text = _header()
    enum = re.search(r"ADMM_L1C_F_XOPT = 1,.*?\};", text, re.S).group(0)
    values = {k: int(v) for k, v in re.findall(r"(ADMM_L1C_F_\w+) = (\d+)", enum)}
    assert len(values) == 8
    for k, v in values.items():
        assert getattr(L, k[len("ADMM_"):]) == v, k
    declared = set(re.findall(r"\b(admm_l1class_\w+)\(", text))
    assert declared == {n for n in L.EXPORTED_SYMBOLS if n.startswith("admm_l1class_")}
    assert len(declared) == 11
    assert re.search(r"#define ADMM_ABI_VERSION 5\b", text) and L.ABI_VERSION == 5


# ----------------------------------------------------------------------------------------------- 4. argument errors
def _data():
    p = R.problem((40, 12), K=2)
    return p["D"], p["ELL"]


@pytest.mark.parametrize("call, message", (
    (lambda ap, D, E: ap.l1classifier(D, E[:-1, 0], 0.1), "rows in argument D"),
    (lambda ap, D, E: ap.l1classifier_multi(D, np.hstack([E, E[:, :1]]), [0.1, 0.2]), "3 columns for 2 fits"),
    (lambda ap, D, E: ap.l1classifier(D, 0.5 * E[:, 0], 0.1), r"labels \+1 and -1"),
    (lambda ap, D, E: ap.l1classifier(D, np.where(E[:, 0] > 0, 1.0, 0.0), 0.1), r"labels \+1 and -1"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(lossfunction="01")), "0-1 loss is not convex"),
    (lambda ap, D, E: ap.l1classifier_multi(D, E, [0.1, 0.2], dict(lossfunction=["hinge", "01"])), "fit 1: lossfunction"),
    (lambda ap, D, E: ap.l1classifier_path(D, E[:, 0], 3, dict(lossfunction="01")), "0-1 loss is not convex"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], -0.1), "fit 0: lambda"),
    (lambda ap, D, E: ap.l1classifier_multi(D, E, [0.1, -1.0]), "fit 1: lambda"),
    (lambda ap, D, E: ap.l1classifier_path(D, E[:, 0], [0.2, np.nan]), "fit 1: lambda"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(l1weights=-np.ones(12))), "l1weights: every weight"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(l1weights=np.ones(11))), "l1weights has 11 entries"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(weights=-np.ones(40))), "weights: every weight"),
    (lambda ap, D, E: ap.l1classifier_multi(D, E, [0.1, 0.2], dict(ridge=[0.1, -1.0])), "fit 1: ridge"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(C=0.0)), "options.C"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(fast=1)), "options.fast is not available"),
    (lambda ap, D, E: ap.l1classifier_multi(D, E, [0.1, 0.2], dict(relax=1.5)), "options.relax is not available"),
    (lambda ap, D, E: ap.l1classifier_path(D, E[:, 0], 4, dict(convtest=1)), "options.convtest is not available"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(adaptive=1)), "options.adaptive is not available"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(comm=object())), "options.comm is not available"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(stopcond="both")), "'standard' stop rule alone"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(xsolve="cg")), "options.xsolve"),
    (lambda ap, D, E: ap.l1classifier(D, E[:, 0], 0.1, dict(z0=np.zeros(40))), "options.z0 does not have 52 entries"),
    (lambda ap, D, E: ap.l1classifier_multi(D, E, [0.1, 0.2], dict(u0=np.zeros((52, 1)))), "options.u0 is not a 52 x 2"),
    (lambda ap, D, E: ap.l1classifier_path(D, E[:, 0], 0), "options.nlambda"),
    (lambda ap, D, E: ap.l1classifier_path(D, E[:, 0], 5, dict(lambda_min_ratio=0.0)), "lambda_min_ratio"),
))
def test_argument_errors(ap, call, message):
    D, E = _data()
    with pytest.raises(ValueError, match=message):
        call(ap, D, E)


def test_lambda_max_of_the_package_is_the_restated_one(ap):
    D, E = _data()
    w = np.linspace(0.5, 2.0, 40)
    lw = np.linspace(0.0, 1.0, 12)  # (one zero weight: left out of the maximum)
    for loss in ("logistic", "hinge", "sqhinge"):
        fit = R.Fit(loss=loss, weights=w, classcost="balanced", l1weights=lw, C=2.0)
        got = ap.l1classifier_lambda_max(D, E[:, 0], fit.options())
        assert got == pytest.approx(R.lambda_max(D, E[:, 0], fit), rel=1e-14)


def test_the_synthetic_problem(ap):
    p = ap.synth.sparse_classifier_problem(3, 200, 50)
    D, ell, x = p["D"], p["ell"], p["testx"]
    assert D.shape == (200, 50) and np.allclose(np.linalg.norm(D, axis=0), 1.0)
    assert set(np.unique(ell)) == {-1.0, 1.0} and 0 < np.count_nonzero(x) <= 15
    assert np.mean(np.where(D @ x >= 0, 1.0, -1.0) == ell) > 0.8
