"""CPU-side checks: the C-ABI library loads and exports every symbol include/admm_engine.h
declares (no compute without a GPU), struct layouts agree, host logic mirrors the reference's
validation, and the product path fails loudly (no CPU fallback) when no device exists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "admm_engine.h")


def _declared_functions():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(admm_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_exported(ap):
    lib = ap._lib.load()
    declared = _declared_functions()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), f"libadmm_hip.so does not export {name}"
    assert sorted(ap._lib.EXPORTED_SYMBOLS) == declared


def test_struct_sizes_and_defaults(ap):
    lib = ap._lib.load()
    o = ap._lib.Options()
    lib.admm_options_default(C.byref(o))
    assert o.struct_size == C.sizeof(ap._lib.Options)
    # admm.m:57-73 defaults
    assert (o.maxiters, o.rho, o.relax, o.abstol, o.reltol) == (1000, 1.0, 1.0, 1e-5, 1e-3)
    assert (o.Hnormtol, o.convtol, o.restart, o.dvaltol) == (1e-6, 1e-10, 0.999, 1e-8)
    d = ap._lib.ProblemDesc()
    lib.admm_problem_desc_default(C.byref(d))
    assert d.struct_size == C.sizeof(ap._lib.ProblemDesc)
    assert lib.admm_abi_version() == ap._lib.ABI_VERSION == 5


def test_enum_values_match_header(ap):
    txt = open(HEADER).read()
    vals = dict((k, int(v)) for k, v in re.findall(r"\b(ADMM_[A-Z0-9_]+)\s*=\s*(-?\d+)", txt))
    L = ap._lib
    assert vals["ADMM_PROB_LASSO"] == L.PROB_LASSO and vals["ADMM_PROB_LAD"] == L.PROB_LAD
    assert vals["ADMM_PROB_HUBERFIT"] == L.PROB_HUBERFIT and vals["ADMM_PROB_LINEARSVM"] == L.PROB_LINEARSVM
    assert vals["ADMM_PROB_QP_BOUNDED"] == L.PROB_QP_BOUNDED and vals["ADMM_PROB_BASISPURSUIT"] == L.PROB_BASISPURSUIT
    assert vals["ADMM_FAST_WEAK"] == L.FAST_WEAK and vals["ADMM_FAST_STRONG"] == L.FAST_STRONG
    assert vals["ADMM_F_FACTOR"] == L.F_FACTOR and vals["ADMM_F_UHATVALS"] == L.F_UHATVALS
    assert vals["ADMM_XSOLVE_INVERSE"] == L.XSOLVE_INVERSE and vals["ADMM_STOP_NONE"] == L.STOP_NONE
    assert vals["ADMM_E_DEVICE"] == L.E_DEVICE


def test_no_cpu_fallback_without_device(ap):
    """Without a HIP device the product path must raise, not compute on the host."""
    if ap._lib.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device behaviour is exercised in the CPU container")
    p = ap.synth.lasso_problem(0, 32, 8)
    with pytest.raises(ap.AdmmError) as ei:
        ap.lasso(p["D"], p["s"], p["lam"], {})
    assert ei.value.code == ap._lib.E_DEVICE
    y = np.zeros(32)
    rc = ap._lib.load().admm_op_gemv_n(ap._lib.as_dp(p["D"]), 32, 8, 32, ap._lib.as_dp(np.ones(8)),
                                       ap._lib.as_dp(y))
    assert rc == ap._lib.E_DEVICE


def _dense_op_calls(ap):
    """(name, call(**overrides) -> rc) for the operator entry points of the symmetric product and the dense setup
    kernels, each with valid small arguments unless overridden"""
    L, dp = ap._lib.load(), ap._lib.as_dp
    n = 4
    M = np.asfortranarray(np.eye(n) * 2.0)
    Ms = np.asfortranarray(np.tile(np.eye(n), (1, 2)))
    x, y = np.ones(n), np.zeros(n)
    X2, Y2 = np.ones((n, 2), order="F"), np.zeros((n, 2), order="F")
    Cm, Xi = np.zeros((n, n), order="F"), np.zeros((n, n), order="F")

    def symv(M=dp(M), n=n, ld=n, x=dp(x), form=1, ncached=-1, parts=1, y=dp(y)):
        return L.admm_op_symv(M, n, ld, x, form, ncached, parts, y)

    def symv_batch(Ms=dp(Ms), n=n, ld=n, K=2, X=dp(X2), ldX=n, ncached=-1, Y=dp(Y2), ldY=n):
        return L.admm_op_symv_batch(Ms, n, ld, K, X, ldX, ncached, Y, ldY)

    def gemm(ta=0, tb=0, M=n, N=n, K=n, A=dp(M), lda=n, B=dp(M), ldb=n, C=dp(Cm), ldc=n, lower=0):
        return L.admm_op_gemm(ta, tb, M, N, K, 1.0, A, lda, B, ldb, 0.0, C, ldc, lower)

    def trtri(Lf=dp(M), n=n, ld=n, X=dp(Xi), ldX=n):
        return L.admm_op_trtri(Lf, n, ld, X, ldX)

    def llt_apply(Lf=dp(M), n=n, ld=n, x=dp(x), y=dp(y)):
        return L.admm_op_llt_apply(Lf, n, ld, x, y)

    keep = (M, Ms, x, y, X2, Y2, Cm, Xi)  # the defaults above hold pointers into these
    return dict(symv=symv, symv_batch=symv_batch, gemm=gemm, trtri=trtri, llt_apply=llt_apply), keep


def test_dense_ops_reject_bad_arguments_before_touching_the_device(ap):
    """E_INVALID for null pointers, ld < rows, and every out-of-range selector -- decided on the host, so the answer is
    the same with and without a device"""
    ops, _keep = _dense_op_calls(ap)
    bad = [
        ("symv", dict(M=None)), ("symv", dict(x=None)), ("symv", dict(y=None)), ("symv", dict(n=0)),
        ("symv", dict(ld=3)), ("symv", dict(form=-1)), ("symv", dict(form=4)), ("symv", dict(parts=0)),
        ("symv", dict(form=0, parts=2)), ("symv", dict(ncached=-2)), ("symv", dict(form=0, n=3, ld=3)),
        ("symv_batch", dict(Ms=None)), ("symv_batch", dict(X=None)), ("symv_batch", dict(Y=None)),
        ("symv_batch", dict(ld=3)), ("symv_batch", dict(ldX=3)), ("symv_batch", dict(ldY=3)),
        ("symv_batch", dict(K=0)), ("symv_batch", dict(ncached=-2)),
        ("gemm", dict(A=None)), ("gemm", dict(B=None)), ("gemm", dict(C=None)), ("gemm", dict(lda=3)),
        ("gemm", dict(ldb=3)), ("gemm", dict(ldc=3)), ("gemm", dict(K=0)), ("gemm", dict(ta=2)), ("gemm", dict(tb=-1)),
        ("gemm", dict(ta=1, K=5, lda=4)), ("gemm", dict(tb=1, N=5, ldb=4)), ("gemm", dict(M=3, lower=1)),
        ("trtri", dict(Lf=None)), ("trtri", dict(X=None)), ("trtri", dict(ld=3)), ("trtri", dict(ldX=3)),
        ("trtri", dict(n=0)),
        ("llt_apply", dict(Lf=None)), ("llt_apply", dict(x=None)), ("llt_apply", dict(y=None)),
        ("llt_apply", dict(ld=3)), ("llt_apply", dict(n=0)),
    ]
    for name, kw in bad:
        assert ops[name](**kw) == ap._lib.E_INVALID, (name, kw)
    for name in ops:
        assert f"admm_op_{name}" in ap._lib.EXPORTED_SYMBOLS


def test_dense_ops_have_no_cpu_fallback(ap):
    """valid arguments: the result of a device, or E_DEVICE -- never a host computation"""
    ops, _keep = _dense_op_calls(ap)
    expected = ap._lib.OK if ap._lib.device_count() > 0 else ap._lib.E_DEVICE
    for name, call in ops.items():
        assert call() == expected, name
    if expected != ap._lib.OK:
        assert b"no CPU fallback" in ap._lib.load().admm_last_error()


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "admm-project_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+\.*oracle\b", src, flags=re.M), f
                assert not re.search(r"import_module\(\s*['\"]oracle", src), f
                assert not re.search(r"#include\s*[<\"][^>\"]*oracle", src), f


def test_admm_handle_validation(ap):
    # caller-supplied handles need a device (they run on CUDA tensors): on a CPU box the engine fails loudly.  With a
    # GPU visible those calls would run (the gpu-marked tests cover that); the argument checks hold everywhere
    no_device = ap._lib.device_count() <= 0
    if no_device:
        with pytest.raises(ap.AdmmError, match="no HIP device"):
            ap.admm(lambda x, z, u, r: x, lambda x, z, u, r: z, dict(A=1, B=-1, c=0, m=4, nA=4, nB=4))
    with pytest.raises(ValueError, match="no number of columns nB"):  # admm.m:206-212
        ap.admm(lambda x, z, u, r: x, lambda x, z, u, r: z, dict(A=1, B=lambda v: v, c=0, m=4, nA=4))
    with pytest.raises(ValueError, match="neither a numeric matrix nor function handle"):  # admm.m:217-222
        ap.admm(lambda x, z, u, r: x, lambda x, z, u, r: z, dict(A=1, B=[1.0, 2.0], c=0, m=4, nA=4))
    if no_device:
        with pytest.raises(ap.AdmmError, match="no HIP device"):  # a general B is engine-native: it needs the device too
            ap.admm(lambda x, z, u, r: x, lambda x, z, u, r: z, dict(A=1, B=np.eye(4), c=0, m=4, nA=4, nB=4))
    with pytest.raises(ValueError, match="options.At must be one too"):  # admm.m:139-158
        ap.admm(lambda x, z, u, r: x, lambda x, z, u, r: z, dict(A=lambda v: v, B=-1, c=0, m=4, nA=4, nB=4))
    if no_device:
        with pytest.raises(ap.AdmmError, match="no HIP device"):  # function-handle operators also need the device
            ap.admm(lambda x, z, u, r: x, lambda x, z, u, r: z,
                    dict(A=lambda v: v, At=lambda v: v, B=-1, c=0, m=4, nA=4, nB=4))
    with pytest.raises(TypeError):
        ap.admm(None, None, "not a struct")
    with pytest.raises(TypeError, match="not a function handle"):
        ap.admm(3, lambda x, z, u, r: z, {})


def test_getproxops_argument_errors(ap):
    with pytest.raises(TypeError):
        ap.getproxops(3, {})
    with pytest.raises(TypeError):
        ap.getproxops("lasso", [])
    with pytest.raises(ValueError):
        ap.getproxops("not-a-solver", {})


def test_solver_validation_mirrors_reference(ap):
    p = ap.synth.lasso_problem(0, 32, 8)
    with pytest.raises(ValueError):  # lasso.m:132
        ap.lasso(p["D"], p["s"], -1.0, {})
    with pytest.raises(ValueError):  # lasso.m:138
        ap.lasso(p["D"], p["s"], 0.1, dict(rho=0.0))
    with pytest.raises(TypeError):
        ap.lasso(p["D"], p["s"], 0.1, None)
    with pytest.raises(ValueError):  # lad.m:119-121
        ap.lad(p["D"], p["s"][:-1], {})
    with pytest.raises(ValueError):  # linearsvm.m:270
        ap.linearsvm(p["D"], np.ones(32), -2.0, {})
    with pytest.raises(ValueError):  # basispursuit.m:195
        ap.basispursuit(p["D"], p["s"], {})


def test_slicemaker_matches_reference_semantics(ap):
    from oracle.solvers_ref import slicemaker as ref

    sm = ap.errorcheck.slicemaker
    for length, workers in ((100000, 8), (100003, 8), (17, 4), (6000, 7), (8, 8)):
        assert sm(0, workers, length) == ref(0, workers, length)
        assert sum(sm(0, workers, length)) == length
    assert sm([4, 6], 2, 10) == ref([4, 6], 2, 10)
    assert sm(3, 2, 10) == ref(3, 2, 10) == [3, 3, 3, 1]
    assert sm(5, 2, 10) == [5, 5]  # q13: the reference zeroes the last slice here; documented deviation
    with pytest.raises(ValueError):
        sm([4, 5], 2, 10)
    assert ap.errorcheck.rank_rows(100003, 2, 8) == (25002, 37503)
    assert ap.errorcheck.slice_ranges([3, 4]) == [(0, 3), (3, 7)]


def test_synth_shapes_and_layout(ap):
    p = ap.synth.lasso_problem(0, 64, 16)
    assert p["D"].flags["F_CONTIGUOUS"] and p["D"].shape == (64, 16)
    np.testing.assert_allclose(np.sum(p["D"] ** 2, axis=0), 1.0, rtol=1e-12)
    assert p["lam"] == pytest.approx(0.1 * np.max(np.abs(p["D"].T @ p["s"])))
    q = ap.synth.lasso_problem(0, 64, 16)
    np.testing.assert_array_equal(p["D"], q["D"])  # seeded
    big = ap.synth.lasso_problem(5, 4096, 1100, threads=4)  # threaded generator path
    np.testing.assert_allclose(np.sum(big["D"] ** 2, axis=0), 1.0, rtol=1e-12)
    s = ap.synth.svm_problem(0, 16, 16)
    assert set(np.unique(s["ell"])) == {-1.0, 1.0}
    t = ap.synth.tv_problem(0, 64)
    assert t["s"].shape == (64,)


def test_row_sharded_generator_matches_full(ap):
    full = ap.synth.lasso_problem(3, 4200, 1001, threads=3)  # large (threaded) path
    parts = [ap.synth.lasso_problem(3, 4200, 1001, threads=2, row_range=ap.errorcheck.rank_rows(4200, r, 3))
             for r in range(3)]
    D = np.concatenate([q["D"] for q in parts], axis=0)
    np.testing.assert_allclose(D, full["D"], rtol=1e-14, atol=1e-16)
    np.testing.assert_allclose(np.concatenate([q["s"] for q in parts]), full["s"], rtol=1e-12, atol=1e-14)
    small = ap.synth.lasso_problem(1, 64, 16, row_range=(10, 30))
    np.testing.assert_array_equal(small["D"], ap.synth.lasso_problem(1, 64, 16)["D"][10:30])


def test_mnist_label_reader(ap, tmp_path):
    import struct

    path = tmp_path / "labels.idx1-ubyte"
    labels = np.arange(20, dtype=np.uint8) % 10
    path.write_bytes(struct.pack(">ii", 2049, 20) + labels.tobytes())
    np.testing.assert_array_equal(ap.synth.read_idx1_labels(str(path), 10), labels[:10])
    img = tmp_path / "img.idx3-ubyte"
    raw = (np.arange(2 * 28 * 28) % 256).astype(np.uint8)
    img.write_bytes(struct.pack(">iiii", 2051, 2, 28, 28) + raw.tobytes())
    X = ap.synth.read_idx3_images(str(img))
    assert X.shape == (2, 400) and X.max() <= 1.0
    np.testing.assert_allclose(X[0, 0], raw.reshape(2, 28, 28)[0, 4, 4] / 255.0)
    bad = tmp_path / "bad"
    bad.write_bytes(struct.pack(">ii", 1234, 1) + b"\0")
    with pytest.raises(ValueError):
        ap.synth.read_idx1_labels(str(bad))


def test_mnist_label_files_the_reference_holds(ap):
    """examples/MNIST/{train,t10k}-labels.idx1-ubyte are the only DATA files in the reference tree (the image files its
    example reads, mnistsvm.m:51-54, are absent there): committed byte for byte under tests/golden/mnist/ and read with
    the loader that mirrors readMNIST (mnistsvm.m:215-233).  Pinned against what is publicly known about MNIST: the
    counts, the class histograms, the first ten labels of either file -- and the +1 / -1 relabelling of trainForDigit
    (mnistsvm.m:133-142)."""
    import os

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mnist")
    train = ap.synth.read_idx1_labels(os.path.join(here, "train-labels.idx1-ubyte"))
    test = ap.synth.read_idx1_labels(os.path.join(here, "t10k-labels.idx1-ubyte"), 10000)
    assert train.shape == (60000,) and test.shape == (10000,)
    assert np.bincount(train.astype(int)).tolist() == [5923, 6742, 5958, 6131, 5842, 5421, 5918, 6265, 5851, 5949]
    assert np.bincount(test.astype(int)).tolist() == [980, 1135, 1032, 1010, 982, 892, 958, 1028, 974, 1009]
    assert train[:10].tolist() == [5, 0, 4, 1, 9, 2, 1, 3, 1, 4] and test[:10].tolist() == [7, 2, 1, 0, 4, 1, 4, 9, 5, 9]
    with pytest.raises(ValueError):  # "Trying to read too many digits" (mnistsvm.m:226-228)
        ap.synth.read_idx1_labels(os.path.join(here, "t10k-labels.idx1-ubyte"), 10001)
    ell = np.where(train == 3, 1.0, -1.0)  # trainForDigit(., ., ., ell, 3)
    assert int((ell > 0).sum()) == 6131 and set(np.unique(ell)) == {-1.0, 1.0}


def test_solver_argument_errors_mirror_the_reference(ap):
    """Validation happens on the host before any device work: the reference's error() texts (model.m:204-211,
    linearprogram.m:241-244, quadraticprogram.m:348-363, lasso.m / lad.m size checks)."""
    z = np.zeros
    with pytest.raises(ValueError, match="rows in P do not match number of rows in Q"):
        ap.model(z((5, 3)), z((4, 3)), z(5), z(4), {})
    with pytest.raises(ValueError, match="columns in P do not match number of columns in Q"):
        ap.model(z((5, 3)), z((5, 2)), z(5), z(5), {})
    with pytest.raises(ValueError, match="rows in P does not match length of vector r"):
        ap.model(z((5, 3)), z((5, 3)), z(4), z(5), {})
    with pytest.raises(ValueError, match="rows in Q does not match length of vector s"):
        ap.model(z((5, 3)), z((5, 3)), z(5), z(6), {})
    with pytest.raises(ValueError, match="columns in D do not match length of vector b"):
        ap.linearprogram(z(4), z((2, 3)), z(2), {})
    with pytest.raises(ValueError, match="rows in D does not match length of vector s"):
        ap.linearprogram(z(3), z((2, 3)), z(5), {})
    with pytest.raises(ValueError, match="both constraint inputs are matrices"):
        ap.quadraticprogram(np.eye(3), z(3), 0.0, z((2, 3)), z((2, 3)), {})
    with pytest.raises(ValueError, match="do not match lengths of P and q"):
        ap.quadraticprogram(np.eye(3), z(3), 0.0, z((2, 4)), z(2), {})
    with pytest.raises(ValueError, match="do not match size of s"):
        ap.lasso(z((5, 3)), z(4), 0.1, {})
    with pytest.raises(ValueError, match="not an image"):
        ap.totalvariation2d(z(7), 1.0, {})
    with pytest.raises(TypeError, match="not a struct"):
        ap.linearprogram(z(3), z((2, 3)), z(2), "options")


def test_single_feature_quirks_of_the_reference_are_reproduced(ap):
    """admm.m:145-148, 151, 188-190: the solvers that hand admm a data matrix as A without options.nA
    (totalvariation.m:151-157, unwrappedadmm.m:81-86, linearsvm.m:221-227) cannot run with a single column -- the
    oracle restates those checks, the mirror raises the same errors (found by tests/sweeps/fuzz_solvers.py: the engine
    itself solves these shapes)."""
    from oracle import solvers_ref as S

    one = np.array([0.7])
    col = np.arange(1.0, 6.0).reshape(5, 1)
    ell = np.array([1.0, -1.0, 1.0, -1.0, 1.0])
    for f in (ap.totalvariation, S.totalvariation):
        with pytest.raises(ValueError, match="(?i)scalar"):
            f(one, 1.0, {})
    for f in (ap.linearsvm, S.linearsvm):
        with pytest.raises(ValueError, match="(?i)rows of At|rows in At"):
            f(col, ell, 1.0, {})
    with pytest.raises(ValueError, match="rows in At"):
        ap.unwrappedadmm(lambda x, z, u, rho: x, col, {})


def _gfx950_disassembly(tmp_path, symbol_part):
    """Disassembly (llvm-objdump) of the shipped library's gfx950 kernels whose mangled name contains `symbol_part`."""
    import shutil
    import subprocess

    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not found")
    so = tmp_path / "libadmm_hip.so"
    shutil.copy(os.path.join(ROOT, "admm-project_amd", "libadmm_hip.so"), so)
    subprocess.run([objdump, "--offloading", str(so)], cwd=tmp_path, check=True, capture_output=True)
    kernels = {}
    for f in sorted(tmp_path.iterdir()):
        if "amdgcn" not in f.name:
            continue
        out = subprocess.run([objdump, "-d", "--no-show-raw-insn", str(f)], capture_output=True, text=True).stdout
        name = None
        for line in out.splitlines():
            if line.endswith(">:"):
                name = line.split("<")[1][:-2]
                name = name if symbol_part in name else None
                if name:
                    kernels[name] = []
            elif name and line.strip():
                kernels[name].append(line.split("//")[0].strip())
    return kernels


def test_hand_issued_stop_load_is_not_read_before_its_wait(tmp_path):
    """tv.hip: the 1-D TV kernels ask for ctrl->stop with a hand-written `s_load_dword` at the top and wait for it
    (`s_waitcnt lgkmcnt(0)`) behind the tile's vector loads; in between the compiler believes the register holds a
    value.  The hardware does not interlock a scalar load: any instruction that READ the register in between (a copy,
    a spill) would see garbage and could make a whole tile return without storing its iterate.  Checked on the code
    that ships: between the load and the first full scalar-memory wait nothing mentions the register."""
    import re

    kernels = _gfx950_disassembly(tmp_path, "tv_direct")
    assert any("tv_direct2_kernel" in k for k in kernels) and any("tv_direct_kernel" in k for k in kernels)
    checked = 0
    for name, ins in kernels.items():
        loads = [(i, s) for i, s in enumerate(ins[:120]) if re.match(r"s_load_dword s\d+, s\[\d+:\d+\], 0x0$", s)]
        assert loads, f"{name}: the hand-issued stop load was not found"
        for i, s in loads:
            reg = int(re.match(r"s_load_dword s(\d+),", s).group(1))
            for later in ins[i + 1:]:
                if later.startswith("s_waitcnt") and ("lgkmcnt(0)" in later or later == "s_waitcnt 0"):
                    break
                singles = [int(v) for v in re.findall(r"\bs(\d+)\b", later)]
                ranges = [(int(a), int(b)) for a, b in re.findall(r"s\[(\d+):(\d+)\]", later)]
                assert reg not in singles and not any(a <= reg <= b for a, b in ranges), (name, s, later)
            else:
                raise AssertionError(f"{name}: no scalar-memory wait behind the stop load")
            checked += 1
    assert checked >= len(kernels)
