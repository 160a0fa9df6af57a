"""The 'lasso' problem with a sparse args.D through the MEX gateway: the gateway forwards MATLAB's sparse
storage as it is, the binding layer describes the sparse engine and the gateway calls admm_engine_create_sparse."""
import numpy as np
import pytest

from mexharness import Harness, MexError, Sparse, build
from sparse_cases import problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex(tmp_path_factory, ap):
    ap._lib.load()
    return Harness(build(tmp_path_factory.mktemp("mexsp")))


def _args(p, **more):
    m, n = p["A"].shape
    args = dict(D=Sparse(p["A"]), s=p["s"], m=m, n=n, parallel=0, rho=1.0, **more)
    args["lambda"] = p["lam"]
    return args


def test_mex_sparse_lasso_matches_the_python_surface(gpu, mex):
    p = problem(gpu, 257, 65, 0.03, seed=322)
    options = dict(objevals=1, A=1, At=1, m=65, nA=65, nB=65, B=-1, c=0, parallel="none")
    got = mex.call("solve", "lasso", _args(p), options, dict(objnative=1, s=p["s"]))
    ref = gpu.lasso(p["D"], p["s"], p["lam"], dict(objevals=1, quiet=1))
    assert ref["xsolve"] == "cg" and ref["nnz"] == p["D"].nnz
    assert int(got["steps"]) == ref["steps"]
    for key in ("xopt", "zopt", "uopt", "objevals", "pnorm", "dnorm"):
        a, b = np.asarray(got[key], dtype=float), np.asarray(ref[key], dtype=float)
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 1e-12 * max(1.0, np.max(np.abs(b))), key


def test_mex_sparse_refusals(gpu, mex):
    p = problem(gpu, 257, 65, 0.03, seed=322)
    options = dict(A=1, At=1, m=65, nA=65, nB=65, B=-1, c=0, parallel="none")
    with pytest.raises(MexError) as err:
        mex.call("solve", "lasso", _args(p, xsolve="trsv"), options)
    assert "matrix-free" in err.value.message
    with pytest.raises(MexError) as err:
        mex.call("solve", "lad", dict(D=Sparse(p["A"]), s=p["s"]), dict(options, m=257, nB=257))
    assert "'lad'" in err.value.message
    got = mex.call("solve", "lasso", _args(p), dict(options, maxiters=3))  # ... and the gateway still works
    assert 1 <= int(got["steps"]) <= 3
