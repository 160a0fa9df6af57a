"""Host side of the multi-fit regression: the exported C ABI, the defaults and sizes of its structs, and
the argument checks of robustfit_multi / quantilereg_multi, which are raised before any device call (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ENTRIES = ("admm_reg_multi_desc_default", "admm_reg_multi_options_default", "admm_reg_multi_create", "admm_reg_multi_run",
           "admm_reg_multi_fetch", "admm_reg_multi_set_weights", "admm_reg_multi_chunk", "admm_reg_multi_destroy")


@pytest.fixture(scope="module")
def lib(ap):
    return ap._lib.load()


def test_symbol_table_holds_the_entries(ap, lib):
    """the dynamic symbol table of the built library, read from the file itself"""
    out = subprocess.run(["nm", "-D", "--defined-only", ap._lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = set(re.findall(r"\bT (admm_[a-z0-9_]+)", out))
    for name in ENTRIES + ("admm_reg_multi_launches",):
        assert name in names, name
        assert name in ap._lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None


def test_abi_version_is_unchanged(lib):
    assert lib.admm_abi_version() == 5


def test_defaults_and_struct_sizes(ap, lib):
    L = ap._lib
    d = L.RegMultiDesc()
    lib.admm_reg_multi_desc_default(C.byref(d))
    assert d.struct_size == C.sizeof(L.RegMultiDesc) == 112
    assert (d.K, d.m, d.n, d.ns, d.mem, d.device) == (1, 0, 0, 1, L.MEM_HOST, 0)
    assert not d.D and not d.S and not d.kind and not d.a and not d.b and not d.epsilon and not d.delta and not d.comm
    o = L.RegMultiOptions()
    lib.admm_reg_multi_options_default(C.byref(o))
    assert o.struct_size == C.sizeof(L.RegMultiOptions) == 88
    assert (o.maxiters, o.rho, o.abstol, o.reltol, o.relax) == (1000, 1.0, 1e-5, 1e-3, 1.0)
    assert (o.fast, o.convtest, o.domaxiters, o.objevals, o.check_every) == (L.FAST_OFF, 0, 0, 0, 0)
    assert not o.x0 and not o.z0 and not o.u0
    assert C.sizeof(L.RegMultiSummary) == 16
    assert 1 <= lib.admm_reg_multi_chunk() <= 10
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "admm_engine.h")).read()
    assert int(re.search(r"#define ADMM_REG_MULTI_MAX_N (\d+)", hdr).group(1)) == L.REG_MULTI_MAX_N == 448
    vals = dict((k, int(v)) for k, v in re.findall(r"\b(ADMM_REGM_F_[A-Z]+)\s*=\s*(\d+)", hdr))
    assert vals == dict(ADMM_REGM_F_XOPT=L.REGM_F_XOPT, ADMM_REGM_F_ZOPT=L.REGM_F_ZOPT, ADMM_REGM_F_UOPT=L.REGM_F_UOPT,
                        ADMM_REGM_F_PNORM=L.REGM_F_PNORM, ADMM_REGM_F_PERR=L.REGM_F_PERR,
                        ADMM_REGM_F_OBJEVALS=L.REGM_F_OBJEVALS)


def _no_device(ap, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device call was made before the arguments were checked")
    monkeypatch.setattr(ap.reg_multi.RegMulti, "__init__", boom)
    monkeypatch.setattr(ap.engine.Engine, "__init__", boom)


def test_argument_errors_come_before_any_device_call(ap, monkeypatch):
    _no_device(ap, monkeypatch)
    rng = np.random.default_rng(0)
    D = rng.random((40, 6))
    s = rng.random(40)
    for taus in ([0.1, 0.0], [0.5, 1.0], [0.2, 1.3], [0.2, np.nan]):
        with pytest.raises(ValueError, match=r"fit 1: tau must lie strictly inside \(0, 1\)"):
            ap.quantilereg_multi(D, s, taus, {})
    with pytest.raises(ValueError, match="sets the slopes itself"):
        ap.quantilereg_multi(D, s, [0.5], dict(tau=0.5))
    five = [dict(kind="lad", tau=t) for t in (0.1, 0.3, 0.5, 0.7, 0.9)]
    with pytest.raises(ValueError, match="S has 3 columns for 5 fits"):
        ap.robustfit_multi(D, rng.random((40, 3)), five, {})
    with pytest.raises(ValueError, match="rows"):
        ap.robustfit_multi(D, rng.random(39), five, {})
    with pytest.raises(ValueError, match="fit 2: slopes must hold two finite values > 0"):
        ap.robustfit_multi(D, s, [dict(kind="lad"), dict(kind="huber"), dict(kind="lad", slopes=(1.0, -0.5))], {})
    with pytest.raises(ValueError, match="fit 1: delta belongs to huberfit, not to lad"):
        ap.robustfit_multi(D, s, [dict(kind="huber", delta=0.5), dict(kind="lad", delta=0.5)], {})
    with pytest.raises(ValueError, match="fit 0: epsilon belongs to lad, not to huberfit"):
        ap.robustfit_multi(D, s, [dict(kind="huber", epsilon=0.5)], {})
    with pytest.raises(ValueError, match="fit 1: tau beside slopes"):
        ap.robustfit_multi(D, s, [dict(kind="lad"), dict(kind="lad", tau=0.5, slopes=(1, 1))], {})
    with pytest.raises(ValueError, match="fit 0: kind"):
        ap.robustfit_multi(D, s, [dict(kind="hinge")], {})
    with pytest.raises(ValueError, match="fit 1: unknown field 'weights'"):
        ap.robustfit_multi(D, s, [dict(kind="lad"), dict(kind="lad", weights=np.ones(40))], {})
    with pytest.raises(ValueError, match="mixed lengths"):
        ap.robustfit_multi(D, s, dict(kind="lad", tau=[0.1, 0.5, 0.9], epsilon=[0.0, 0.1]), {})
    with pytest.raises(ValueError, match="fits is neither"):
        ap.robustfit_multi(D, s, [], {})
    with pytest.raises(ValueError, match="weights has 39 entries"):
        ap.robustfit_multi(D, s, five, dict(weights=np.ones(39)))
    with pytest.raises(ValueError, match="x0 is not a 6 x 5 matrix"):
        ap.robustfit_multi(D, s, five, dict(x0=np.zeros((6, 4))))
    for key, val in (("relax", 1.5), ("fast", 1), ("convtest", 1), ("stopcond", "hnorm")):
        with pytest.raises(ValueError, match=key):
            ap.robustfit_multi(D, s, five, {key: val})
    with pytest.raises(TypeError):
        ap.robustfit_multi(D, s, five, "options")
    # good arguments pass, in both spellings of fits, and the first device call is reached
    with pytest.raises(AssertionError, match="device call"):
        ap.robustfit_multi(D, rng.random((40, 5)), five, dict(weights=np.ones(40)))
    with pytest.raises(AssertionError, match="device call"):
        ap.robustfit_multi(D, s, dict(kind="lad", tau=[0.1, 0.5, 0.9]), {})
    with pytest.raises(AssertionError, match="device call"):
        ap.quantilereg_multi(D, s, [0.25, 0.75], {})


def test_the_wide_fallback_is_checked_the_same_way(ap, monkeypatch):
    """n > 448 runs the single solvers: the argument errors are the same, and the first device call is an Engine"""
    _no_device(ap, monkeypatch)
    rng = np.random.default_rng(1)
    D = rng.random((460, 449))
    s = rng.random(460)
    with pytest.raises(ValueError, match="fit 0: tau"):
        ap.quantilereg_multi(D, s, [1.5], {})
    with pytest.raises(AssertionError, match="device call"):
        ap.quantilereg_multi(D, s, [0.5], {})
