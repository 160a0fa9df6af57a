"""The one-launch tail behind the packed lower-triangle x-solve on its own grid: workgroups of 64 elements x 8 slots
(loop_kernels.hip: kTailTileWide), two per 128-element tile of the x-solve, each element's partial rows split into eight
shares that are added in slot order.

Shapes: the packed path starts at n = 1536 (consensus.h: kSymvHalfMin), twelve tiles, which is also a multiple of 128;
1537 leaves the last workgroup one element; 1599 and 1601 have n mod 128 = 63 and 65, one below and one above the
tail's tile (the last workgroup is one element short of full / the second workgroup of the last x-solve tile holds
one element); 1664 is the next multiple of 128.  Every shape has several workgroups per tile row and m = 2n."""
import numpy as np
import pytest

from oracle import solvers_ref as S

pytestmark = pytest.mark.gpu

TOL = 1e-9
ITERS = 15
SHAPES = [1536, 1537, 1599, 1601, 1664]
HIST = ("xvals", "zvals", "uvals", "pnorm", "dnorm", "perr", "derr")


def _err(name, got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert not np.isnan(got).any() and not np.isnan(ref).any(), f"{name}: NaN"
    if ref.ndim == 1:  # scalar histories: per entry, as tests/test_gpu_parity.py compares them
        scale = np.maximum(np.abs(ref), 1e-12 + 1e-3 * np.max(np.abs(ref)))
        return float(np.max(np.abs(got - ref) / scale))
    return float(np.max(np.abs(got - ref)) / max(1e-300, np.max(np.abs(ref))))


def _packed_inverse(n, info, storage):
    """the explicit inverse, stored as the tiles of its lower triangle (fp64 or compact): never the padded square"""
    t = (n + 127) // 128
    return info["xsolve_used"] == "inverse" and 0 < storage["stored_bytes"] <= 8 * 128 * 128 * t * (t + 1) // 2


@pytest.mark.parametrize("n", SHAPES)
def test_lasso_15_iterations_against_the_oracle(gpu, n):
    p = gpu.synth.lasso_problem(n, 2 * n, n)
    o = dict(maxiters=ITERS, domaxiters=1)
    got = gpu.lasso(p["D"], p["s"], p["lam"], dict(o, xsolve="inverse", record_history=1))
    assert _packed_inverse(n, got["engine_info"], got["xsolve_storage"]), (got["engine_info"], got["xsolve_storage"])
    ref = S.lasso(p["D"], p["s"], p["lam"], o)
    assert got["steps"] == ref["steps"] == ITERS
    for k in HIST:
        err = _err(k, got[k], ref[k])
        print(f"n = {n} {k}: relative error {err:.3e} (bound {TOL:g})")
        assert err < TOL, (k, err)


def _run(gpu, eng, n):
    L = gpu._lib
    st = eng.run(maxiters=ITERS, domaxiters=1, record_history=1)
    assert st.steps == ITERS
    out = {k: eng.fetch(f, n * ITERS, (n, ITERS)) for k, f in (("xvals", L.F_XVALS), ("zvals", L.F_ZVALS),
                                                              ("uvals", L.F_UVALS))}
    out.update({k: eng.fetch(f, ITERS) for k, f in (("pnorm", L.F_PNORM), ("dnorm", L.F_DNORM), ("perr", L.F_PERR),
                                                    ("derr", L.F_DERR))})
    return out


def test_repeat_penalty_and_group_tails_on_one_engine(gpu):
    """n = 1601 on one engine: a second run is bitwise the first; weighted l1 with unit weights (penalty_prox_fin_kernel)
    and singleton groups (group_prox_fin_kernel) are the plain lasso -- to 1e-12 over the histories, as
    tests/test_gpu_grouplasso.py compares singleton groups, and BITWISE in the x of the first iteration, which is nothing
    but the sum of the x-solve's partial rows of one right-hand side: the three kernels take the same shares in the same
    order."""
    L = gpu._lib
    n = 1601
    p = gpu.synth.lasso_problem(n, 2 * n, n)
    eng = gpu.Engine(L.PROB_LASSO, D=p["D"], s=p["s"], lam=p["lam"], xsolve=L.XSOLVE_INVERSE)
    try:
        assert _packed_inverse(n, eng.info(), eng.xsolve_storage())
        plain = _run(gpu, eng, n)
        again = _run(gpu, eng, n)
        for k in HIST:
            assert np.array_equal(again[k], plain[k]), k  # fixed summation order: bitwise reproducible
        eng.set_penalty(np.ones(n))
        assert eng.penalty()["has_l1weights"]
        pen = _run(gpu, eng, n)
        eng.set_penalty(None)
        eng.set_groups([1] * n)
        assert eng.info()["ngroups"] == n
        grp = _run(gpu, eng, n)
        eng.set_groups(None)
        back = _run(gpu, eng, n)
    finally:
        eng.close()
    for name, other in (("unit weights", pen), ("singleton groups", grp)):
        assert np.array_equal(other["xvals"][:, 0], plain["xvals"][:, 0]), name
        for k in HIST:
            err = _err(k, other[k], plain[k])
            print(f"{name} {k}: relative difference {err:.3e} (bound 1e-12)")
            assert err < 1e-12, (name, k, err)
    for k in HIST:
        assert np.array_equal(back[k], plain[k]), k
