"""The cases of the multi-fit covariance selection tests (tests/test_covsel_multi_host.py on the CPU,
tests/test_gpu_covsel_multi.py on the device), and their per-fit reference: the unchanged oracle loop driven by the
restated closures of tests/covsel_restated.py, one run per (lambda_k, rho_k).  References are computed once per process
and shared; nobody writes to them."""
from __future__ import annotations

import functools

import numpy as np

from covsel_restated import cov, oracle_run, samples

# samples(seed, m, n) -> the steps of the seven fits of grid() at rho = 1, defaults otherwise (recorded from the oracle;
# tests/test_covsel_multi_host.py checks them and that no stop is a knife edge)
CASES = {
    (5, 256, 32): (46, 31, 22, 15, 17, 26, 36),
    (11, 120, 24): (43, 31, 23, 14, 22, 32, 44),
    (3, 400, 96): (36, 28, 24, 16, 18, 30, 46),
}
PER_FIT_RHO = (0.1, 0.3, 1.0, 1.0, 3.0, 10.0, 1.0)
HISTS = ("pnorm", "perr", "dnorm", "derr", "objevals")


def lambda_max(S):
    """max over i != j of |S_ij|: at and above it the fit is diagonal"""
    off = np.abs(S - np.diag(np.diag(S)))
    return float(off.max()) if off.size else 0.0


def grid(S, count=7):
    return lambda_max(S) * np.logspace(0.0, -2.0, count)


@functools.lru_cache(maxsize=None)
def case_S(case):
    S = cov(samples(*case))
    S.setflags(write=False)
    return S


def _freeze(res):
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _oracle(key, lam, rho, extra):
    S = case_S(key) if isinstance(key, tuple) and len(key) == 3 else _EXTRA_S[key]
    return _freeze(oracle_run(np.array(S), lam, dict(dict(extra), rho=rho)))


_EXTRA_S = {}


def oracle_fit(key, lam, rho=1.0, S=None, **options):
    """the oracle's run of one fit, cached: ``key`` a case of CASES, or any hashable name with its ``S``"""
    if S is not None:
        _EXTRA_S.setdefault(key, S)
    return _oracle(key, float(lam), float(rho), tuple(sorted(options.items())))


def df_of(Z):
    """off-diagonal pairs i < j with z_ij != 0 of an n x n matrix (or its n^2 flattening)"""
    Z = np.asarray(Z)
    n = int(round(np.sqrt(Z.size)))
    Z = Z.reshape((n, n), order="F")
    return int(np.count_nonzero(Z[np.triu_indices(n, k=1)]))


def knife_margin(ref):
    """(how far below their tolerances both residuals are at the last step, how far above the worse one is at the step
    before), each relative: > 0 on both means the stop is no knife edge"""
    s = int(ref["steps"])
    p, pe, d, de = (np.asarray(ref[k], dtype=np.float64) for k in ("pnorm", "perr", "dnorm", "derr"))
    last = min((pe[s - 1] - p[s - 1]) / pe[s - 1], (de[s - 1] - d[s - 1]) / de[s - 1])
    before = max((p[s - 2] - pe[s - 2]) / pe[s - 2], (d[s - 2] - de[s - 2]) / de[s - 2]) if s >= 2 else np.inf
    return float(last), float(before)


# more workgroups than CUs, several per CU: K = 300 fits of a small n, every one run to its own stop
MANY_SAMPLES, MANY_K = (77, 64, 8), 300


def many_case():
    S = case_S(MANY_SAMPLES)
    return S, lambda_max(S) * np.logspace(0.0, -2.0, MANY_K)
