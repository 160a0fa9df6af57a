"""Host side of the one-vs-rest linear SVM: the exported C ABI, the defaults of its two structs, and the argument
checks of linearsvm_ovr, which are raised before any device call (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib(ap):
    return ap._lib.load()


def test_library_exports_the_ovr_entry_points(ap, lib):
    for name in ("admm_svm_ovr_create", "admm_svm_ovr_run", "admm_svm_ovr_fetch", "admm_svm_ovr_destroy"):
        assert name in ap._lib.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None


def test_abi_version_is_unchanged(lib):
    assert lib.admm_abi_version() == 5


def test_default_filling_functions(ap, lib):
    L = ap._lib
    d = L.SvmOvrDesc()
    lib.admm_svm_ovr_desc_default(C.byref(d))
    assert d.struct_size == C.sizeof(L.SvmOvrDesc)
    assert (d.K, d.m, d.n, d.mem, d.device) == (1, 0, 0, L.MEM_HOST, 0)
    assert not d.D and not d.ELL and not d.loss and not d.Dplus and not d.comm
    o = L.SvmOvrOptions()
    lib.admm_svm_ovr_options_default(C.byref(o))
    assert o.struct_size == C.sizeof(L.SvmOvrOptions)
    assert (o.maxiters, o.rho, o.abstol, o.reltol, o.Hnormtol) == (1000, 1.0, 1e-5, 1e-3, 1e-6)
    assert (o.relax, o.fast, o.convtest, o.domaxiters, o.objevals, o.check_every) == (1.0, L.FAST_OFF, 0, 0, 0, 0)
    assert not o.x0 and not o.z0 and not o.u0
    assert 1 <= lib.admm_svm_ovr_chunk() <= 32


def _no_device(ap, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device call was made before the arguments were checked")
    monkeypatch.setattr(ap.engine.SvmOvr, "__init__", boom)
    monkeypatch.setattr(ap.engine.Engine, "__init__", boom)


def test_argument_errors_come_before_any_device_call(ap, monkeypatch):
    _no_device(ap, monkeypatch)
    rng = np.random.default_rng(0)
    D = rng.random((40, 6))
    labels = rng.integers(0, 3, size=40).astype(np.float64)
    with pytest.raises(ValueError, match="sizes incompatible"):
        ap.linearsvm_ovr(D, labels[:39], 0.5, {})
    with pytest.raises(ValueError, match="lossfunction"):
        ap.linearsvm_ovr(D, labels, 0.5, dict(lossfunction=["hinge", "01"]))
    with pytest.raises(ValueError, match="x0"):
        ap.linearsvm_ovr(D, labels, 0.5, dict(x0=np.zeros((6, 2))))
    with pytest.raises(ValueError, match="z0"):
        ap.linearsvm_ovr(D, labels, 0.5, dict(z0=np.zeros((39, 3))))
    with pytest.raises(ValueError, match="nonnegative"):
        ap.linearsvm_ovr(D, labels, -1.0, {})
    with pytest.raises(ValueError, match="classes"):
        ap.linearsvm_ovr(D, labels, 0.5, dict(classes=np.zeros((2, 2))))
    with pytest.raises(TypeError):
        ap.linearsvm_ovr(D, labels, 0.5, "options")
    # a class with no member is allowed (all labels -1): the arguments pass, and the first device call is reached
    with pytest.raises(AssertionError, match="device call"):
        ap.linearsvm_ovr(D, labels, 0.5, dict(classes=[0.0, 7.0]))


def test_label_matrix_from_the_reference_label_file(ap):
    labels = ap.synth.reference_mnist_labels("train")
    assert labels is not None and labels.size == 60000
    ELL = ap.solvers.ovr_label_matrix(labels, [3, 7])
    assert ELL.shape == (60000, 2) and ELL.flags.f_contiguous
    for c, digit in enumerate((3, 7)):
        assert np.array_equal(ELL[:, c], np.where(labels == digit, 1.0, -1.0))
    assert set(np.unique(ELL)) == {-1.0, 1.0}
    empty = ap.solvers.ovr_label_matrix(labels, [11])
    assert (empty == -1.0).all()
