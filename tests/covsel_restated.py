"""Covariance selection restated from the reference's formulas, for the tests: the two closures of getProxOps.m:750
(z: soft threshold at lambda/rho) and 1487-1495 (x: the eigen-step of rho*(z - u) - S, here with numpy's eigh) and
the solver's objective (covarianceselection.m:169), driving the unchanged oracle loop (oracle.admm_ref) on the
n^2-flattening of the n x n iterates with A = 1, B = -1, c = 0."""
from __future__ import annotations

import numpy as np

from oracle import admm_ref


def xprox(S, z, u, rho):
    """x = Q*diag((e + sqrt(e.^2 + 4*rho))./(2*rho))*Q' with [Q, E] = eig(rho*(z - u) - S), on n x n matrices."""
    e, Q = np.linalg.eigh(rho * (z - u) - S)
    return Q @ np.diag((e + np.sqrt(e * e + 4.0 * rho)) / (2.0 * rho)) @ Q.T


def closures(S, lam):
    n = S.shape[0]

    def xminf(x, z, u, rho):
        return xprox(S, z.reshape((n, n), order="F"), u.reshape((n, n), order="F"), rho).reshape(-1, order="F")

    def zming(x, z, u, rho):
        v = x + u
        return np.sign(v) * np.maximum(np.abs(v) - lam / rho, 0.0)

    def obj(x, z):
        X = x.reshape((n, n), order="F")
        return np.trace(S @ X) - np.log(np.linalg.det(X)) + lam * np.sum(np.abs(z))

    return xminf, zming, obj


def oracle_run(S, lam, options):
    n = S.shape[0]
    xminf, zming, obj = closures(S, lam)
    o = dict(options, A=1, B=-1, c=0, m=n * n, nA=n * n, nB=n * n, obj=obj)
    return admm_ref.admm(xminf, zming, o)


def samples(seed, m, n, mean=0.0):
    """m Gaussian samples of n correlated variables (a random SPD covariance), column means around `mean`."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    C = G @ G.T / n + 0.5 * np.eye(n)
    D = rng.standard_normal((m, n)) @ np.linalg.cholesky(C).T + mean
    return np.asfortranarray(D)


def cov(D):
    S = np.atleast_2d(np.cov(D, rowvar=False))
    return 0.5 * (S + S.T)
