"""Group lasso without a device: the restatement (tests/grouplasso_restated.py) pinned on its own -- a closed form and
the KKT conditions -- then what the binding layer and ap.grouplasso refuse before any device work, and the ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grouplasso_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------ the restatement, by itself
def test_orthonormal_columns_give_the_closed_form():
    """D'D = I: 1/2*||Dx - s||^2 = 1/2*||x - D's||^2 + const, so the minimiser is the block soft threshold of D's"""
    rng = np.random.default_rng(0)
    Q, _ = np.linalg.qr(rng.standard_normal((96, 40)))
    sizes = [1, 7, 12, 20]
    w = np.array([1.0, 0.5, 2.0, 1.5])
    s = Q @ rng.standard_normal(40) + 0.1 * rng.standard_normal(96)
    lam = 0.4
    exact = R.shrink(Q.T @ s, sizes, lam, w)
    assert np.any(exact == 0.0) and np.any(exact != 0.0)
    r = R.run(Q, s, lam, sizes, dict(abstol=1e-12, reltol=0.0, maxiters=5000), weights=w)
    assert r["steps"] < 5000
    for key in ("xopt", "zopt"):
        err = float(np.max(np.abs(r[key] - exact)))
        print(f"{key}: max error against the closed form {err:.3e}")
        assert err <= 1e-8


def test_kkt_conditions_at_the_restatement_s_solution():
    """0 in D_g'(Dx - s) + lambda*w_g*d||x_g||: a zero group has ||D_g'(s - Dx)|| <= lambda*w_g, a non-zero one
    D_g'(s - Dx) = lambda*w_g*x_g/||x_g||"""
    rng = np.random.default_rng(1)
    m, n = 120, 60
    D = rng.standard_normal((m, n)) / np.sqrt(m)
    sizes = [5, 10, 1, 14, 10, 20]
    off = R.offsets(sizes)
    w = np.sqrt(np.asarray(sizes, dtype=np.float64))
    xt = np.zeros(n)
    xt[off[1]:off[2]] = rng.standard_normal(10)
    xt[off[3]:off[4]] = rng.standard_normal(14)
    s = D @ xt + 0.05 * rng.standard_normal(m)
    g0 = D.T @ s
    lam = 0.3 * max(np.linalg.norm(g0[off[g]:off[g + 1]]) / w[g] for g in range(len(sizes)))
    r = R.run(D, s, lam, sizes, dict(abstol=1e-13, reltol=0.0, maxiters=20000), weights=w)
    assert r["steps"] < 20000
    x = r["zopt"]  # (the iterate that carries the exact zeros)
    grad = D.T @ (s - D @ x)
    zero = nonzero = 0
    for g in range(len(sizes)):
        xg, gg = x[off[g]:off[g + 1]], grad[off[g]:off[g + 1]]
        if not np.any(xg):
            zero += 1
            assert np.linalg.norm(gg) <= lam * w[g] * (1 + 1e-6), g
        else:
            nonzero += 1
            err = float(np.max(np.abs(gg - lam * w[g] * xg / np.linalg.norm(xg))))
            print(f"group {g}: stationarity error {err:.3e}")
            assert err <= 1e-6, g
    assert zero >= 1 and nonzero >= 1, (zero, nonzero)


def test_shrink_form():
    """t = 0 returns v bit for bit; an all-zero group stays zero without a division"""
    v = np.random.default_rng(2).standard_normal(11)
    v[3:7] = 0.0
    with np.errstate(all="raise"):
        assert np.array_equal(R.shrink(v, [3, 4, 4], 0.0), v)
        out = R.shrink(v, [3, 4, 4], 0.5)
    assert np.array_equal(out[3:7], np.zeros(4))
    ld = R.shrink(v, [3, 4, 4], 0.5, dtype=np.longdouble)
    assert ld.dtype == np.longdouble and np.allclose(out, ld.astype(np.float64), rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------ binding layer (no device)
def _binding(ap, **extra):
    from admm_project_amd.binding import Binding
    rng = np.random.default_rng(3)
    args = dict(D=rng.standard_normal((12, 8)), s=rng.standard_normal(12), rho=1.0)
    args["lambda"] = 0.1
    args.update(extra)
    return Binding("lasso", args)


@pytest.mark.parametrize("extra,code", [
    (dict(groups=[3, 4]), "E_INVALID"),                                  # the sizes do not sum to n = 8
    (dict(groups=[3, 0, 5]), "E_INVALID"),                               # a zero size
    (dict(groups=[2.5, 5.5]), "E_INVALID"),                              # a non-integer size
    (dict(groups=[3, 5], groupweights=[1.0, 2.0, 3.0]), "E_INVALID"),    # weights-length mismatch
    (dict(groups=[3, 5], groupweights=[1.0, -2.0]), "E_INVALID"),        # a negative weight
    (dict(groups=[3, 5], groupweights=[1.0, float("inf")]), "E_INVALID"),
    (dict(groupweights=[1.0, 2.0]), "E_INVALID"),                        # weights without groups
    (dict(groups=[3, 5], parallel=1, slices=[6, 6]), "E_UNSUPPORTED"),   # consensus lasso has no groups
], ids=["sum", "zero", "fraction", "count", "negative", "inf", "orphan-weights", "parallel"])
def test_binding_refuses(ap, extra, code):
    with pytest.raises(ap.AdmmError) as ei:
        _binding(ap, **extra)
    assert ei.value.code == getattr(ap._lib, code), str(ei.value)
    assert "group" in str(ei.value)


def test_binding_accepts_a_valid_pair(ap):
    for extra in (dict(groups=[3, 5]), dict(groups=[1, 1, 6], groupweights=[0.0, 1.0, np.sqrt(6.0)])):
        b = _binding(ap, **extra)
        assert b.info()["problem"] == ap._lib.PROB_LASSO and b.info()["nA"] == 8
        b.close()


# ------------------------------------------------------------------------------------ ap.grouplasso (Python checks)
@pytest.mark.parametrize("groups,opts,exc", [
    ([3, 4], {}, ValueError),
    ([3, 0, 5], {}, ValueError),
    ([2.5, 5.5], {}, ValueError),
    ([3, 5], dict(groupweights=[1.0, 2.0, 3.0]), ValueError),
    ([3, 5], dict(groupweights=[1.0, -2.0]), ValueError),
    ([3, 5], dict(parallel="both"), ValueError),
], ids=["sum", "zero", "fraction", "count", "negative", "parallel"])
def test_grouplasso_raises_in_python(ap, monkeypatch, groups, opts, exc):
    """before getproxops is reached: nothing here may touch the library"""
    import admm_project_amd.solvers as S
    monkeypatch.setattr(S, "getproxops", lambda *a, **k: pytest.fail("getproxops was reached"))
    rng = np.random.default_rng(4)
    with pytest.raises(exc):
        ap.grouplasso(rng.standard_normal((12, 8)), rng.standard_normal(12), 0.1, groups, opts)
    with pytest.raises(TypeError):
        ap.grouplasso(rng.standard_normal((12, 8)), rng.standard_normal(12), 0.1, [3, 5], None)


def test_getproxops_checks_groups_before_the_engine(ap, monkeypatch):
    import admm_project_amd.api as A
    monkeypatch.setattr(A, "Engine", lambda *a, **k: pytest.fail("an engine was created"))
    args = dict(D=np.zeros((12, 8)), s=np.zeros(12), groups=[3, 4])
    args["lambda"] = 0.1
    with pytest.raises(ValueError):
        ap.getproxops("LASSO", args)
    args.update(groups=[3, 5], parallel=1, slices=[6, 6])
    with pytest.raises(ap.AdmmError) as ei:
        ap.getproxops("LASSO", args)
    assert ei.value.code == ap._lib.E_UNSUPPORTED


# ------------------------------------------------------------------------------------ ABI
SIZES = dict(admm_problem_desc=272, admm_options=136, admm_run_summary=32, admm_engine_info_t=120, admm_field=64,
             admm_binding_info=64, admm_result_field=40, admm_svm_ovr_desc=88, admm_svm_ovr_options=96,
             admm_svm_ovr_summary=16)


def test_abi_version_and_struct_sizes(ap, tmp_path):
    """ABI 5 and no struct of the header changed its size: the header through a C compiler, the ctypes mirror beside it"""
    L = ap._lib
    assert L.load().admm_abi_version() == L.ABI_VERSION == 5
    mirror = dict(admm_problem_desc=L.ProblemDesc, admm_options=L.Options, admm_run_summary=L.RunSummary,
                  admm_engine_info_t=L.EngineInfo, admm_field=L.Field, admm_binding_info=L.BindingInfo,
                  admm_result_field=L.ResultField, admm_svm_ovr_desc=L.SvmOvrDesc, admm_svm_ovr_options=L.SvmOvrOptions,
                  admm_svm_ovr_summary=L.SvmOvrSummary)
    for name, size in SIZES.items():
        assert C.sizeof(mirror[name]) == size, name
    assert L.EngineInfo.ngroups.offset == L.EngineInfo.obj_form_literal.offset + 4
    src = tmp_path / "sizes.c"
    lines = "\n".join(f'  printf("{n} %zu\\n", sizeof({n}));' for n in SIZES)
    src.write_text('#include <stdio.h>\n#include "admm_engine.h"\nint main(void) {\n'
                   f'  printf("abi %d\\n", ADMM_ABI_VERSION);\n{lines}\n  return 0;\n}}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("abi")) == 5
    assert {k: int(v) for k, v in out.items()} == SIZES
    assert "admm_engine_set_groups" in L.EXPORTED_SYMBOLS and "admm_op_group_soft_threshold" in L.EXPORTED_SYMBOLS
