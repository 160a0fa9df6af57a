"""Covariance selection: a reference for the eigen-step that is exact, or carries a stated error bound, at the inputs
where a symmetric eigen-step goes wrong (tests/covsel_restated.py is the parity restatement; this is the yardstick).

- Matrices with an exactly known spectrum: Q = P * blockdiag(H_a / sqrt(a)) * diag(+-1), H_a Sylvester-Hadamard,
  a in {1, 4, 16, 64, 256, 1024}, P a permutation.  Every entry is +-2^-k, so Q'Q = I exactly, and for eigenvalues on
  the grid 2^-20 * Z with |s| <= 2^20 every partial sum of S = (Q*s) @ Q' is a multiple of 2^-30 below 2^21 in
  magnitude: S is formed without rounding, exactly symmetric, with spectrum exactly s.
- X = f(M) for such a matrix from mpmath: inside a block, (H diag(f) H')_ij = (H f)_{i xor j}, so one Walsh-Hadamard
  transform of f (40 digits) per block gives every entry of X, rounded once.  -log det X = -sum log f in mpmath.
- For an arbitrary symmetric M: eigh(M, UPLO='L') with the stable f, and the bound of `x_bound` (no flat rtol).
- cov(D): two-pass in long double, with the dot-product bound of `cov_bound`.
"""
from __future__ import annotations

import math

import mpmath
import numpy as np

EPS = float(np.finfo(np.float64).eps)
DPS = 40  # mpmath digits: f, the transforms and the log-determinant carry ~2^-130 relative error

# The one constant of every bound here, fixed before the device ran.  Both the device and the reference (LAPACK eigh,
# one n-term product for V f V') make errors of the form (a few) * n * eps * (L * ||M||_F + ||X||_F): one-sided and
# two-sided Jacobi are backward stable with O(n * eps) per converged decomposition, and each entry of V f V' is an
# n-term dot product.  4 covers both sides (device + reference: 2) with a factor 2 for the large path's shift sigma,
# which is at most the Gershgorin radius <= sqrt(n) * ||M||_2 <= sqrt(n) * ||M||_F.
C = 4.0

BLOCKS = (1024, 256, 64, 16, 4, 1)
GRID = 2.0 ** -20  # eigenvalue grid
SMAX = 2.0 ** 20  # eigenvalue magnitude limit


# ---------------------------------------------------------------------------------------------------- the function
def f_stable(lam, rho):
    """f(l) = (l + sqrt(l^2 + 4 rho)) / (2 rho), as the kernel evaluates it: 2 / (sqrt(l^2 + 4 rho) - l) for l < 0."""
    lam = np.asarray(lam, dtype=np.float64)
    r = np.sqrt(lam * lam + 4.0 * rho)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(lam >= 0.0, (lam + r) / (2.0 * rho), 2.0 / (r - lam))


def f_literal(lam, rho):
    """The literal form of getProxOps.m:1494 (cancels for l << -sqrt(rho))."""
    lam = np.asarray(lam, dtype=np.float64)
    return (lam + np.sqrt(lam * lam + 4.0 * rho)) / (2.0 * rho)


def fprime(lam, rho):
    """f'(l) = (1 + l / sqrt(l^2 + 4 rho)) / (2 rho) = f(l) / sqrt(l^2 + 4 rho): positive, increasing (f is convex)."""
    lam = np.asarray(lam, dtype=np.float64)
    return f_stable(lam, rho) / np.sqrt(lam * lam + 4.0 * rho)


def f_mp(lam, rho):
    """f at DPS digits, for one eigenvalue (a float, exact on entry) and rho."""
    with mpmath.workdps(DPS):
        l, r = mpmath.mpf(float(lam)), mpmath.mpf(float(rho))
        return (l + mpmath.sqrt(l * l + 4 * r)) / (2 * r)


# ---------------------------------------------------------------------------------------------------- exact matrices
def hadamard(a):
    """Sylvester-Hadamard matrix of order a (a power of 2), entries +-1."""
    H = np.ones((1, 1))
    while H.shape[0] < a:
        H = np.block([[H, H], [H, -H]])
    return H


def block_sizes(n):
    """n as a sum of block orders from BLOCKS, largest first."""
    out, left = [], n
    for a in BLOCKS:
        while left >= a:
            out.append(a)
            left -= a
    return out


class Exact:
    """Q = P * blockdiag(H_a / sqrt(a)) * diag(+-1) and S = Q diag(s) Q' (exact), for a spectrum s on the grid."""

    def __init__(self, s, seed):
        s = np.asarray(s, dtype=np.float64)
        assert np.all(np.abs(s) <= SMAX) and np.all(s / GRID == np.round(s / GRID)), "s must lie on the 2^-20 grid"
        n = s.size
        rng = np.random.default_rng(seed)
        self.n, self.s = n, s
        self.sizes = block_sizes(n)
        self.perm = rng.permutation(n)  # row i of Q is row perm[i] of the block-diagonal matrix
        self.signs = rng.choice([-1.0, 1.0], size=n)
        Bd = np.zeros((n, n))
        o = 0
        for a in self.sizes:
            Bd[o:o + a, o:o + a] = hadamard(a) / math.sqrt(a)  # sqrt(a) = 2^k: exact
            o += a
        self.Q = Bd[self.perm, :] * self.signs
        self.S = (self.Q * s) @ self.Q.T

    def X(self, lamM, rho):
        """f(M) for M = Q diag(lamM) Q' (lamM exact on the grid: -s for M = -S), each entry rounded once from DPS
        digits; also returns -log det X and trace(S X) at DPS digits and the mp values of f (block order)."""
        n = self.n
        fm = [f_mp(l, rho) for l in lamM]
        Y = np.zeros((n, n))
        o = 0
        with mpmath.workdps(DPS):
            for a in self.sizes:
                g = list(fm[o:o + a])
                h = 1
                while h < a:  # in-place Walsh-Hadamard transform (Sylvester order)
                    for i in range(0, a, 2 * h):
                        for j in range(i, i + h):
                            x, y = g[j], g[j + h]
                            g[j], g[j + h] = x + y, x - y
                    h *= 2
                gd = np.array([float(v / a) for v in g])
                idx = np.arange(a)
                Y[o:o + a, o:o + a] = gd[idx[:, None] ^ idx[None, :]]
                o += a
            logdet = mpmath.fsum(mpmath.log(v) for v in fm)
            trSX = mpmath.fsum(mpmath.mpf(float(si)) * v for si, v in zip(self.s, fm))
        # (column signs cancel in Q diag(f) Q'; the row permutation moves rows and columns alike)
        X = Y[np.ix_(self.perm, self.perm)]
        return X, -logdet, trSX, fm


def spectrum(kind, n, seed):
    """Eigenvalues of S on the 2^-20 grid for the named hard cases."""
    rng = np.random.default_rng(seed)
    grid = lambda v: np.clip(np.round(np.asarray(v, dtype=np.float64) / GRID) * GRID, -SMAX, SMAX)
    if kind == "equal":
        return np.full(n, 0.75)
    if kind == "half-repeated":
        s = grid(rng.uniform(-2.0, 2.0, n))
        s[: n // 2] = s[0]
        return s
    if kind == "quarter-repeated":
        s = grid(rng.uniform(-2.0, 2.0, n))
        s[: n // 4] = s[0]
        return s
    if kind == "zeros":
        s = grid(rng.uniform(-1.0, 1.0, n))
        s[: (3 * n) // 4] = 0.0
        return s
    if kind == "all-zero":
        return np.zeros(n)
    if kind == "range":  # dynamic range 2^+-20, both signs
        return grid(rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(-20.0, 20.0, n))
    if kind == "mixed":
        return grid(rng.uniform(-4.0, 4.0, n))
    if kind == "cluster":  # eigenvalues 2^-20 apart in three clusters
        base = np.array([-1.0, 0.25, 3.0])[rng.integers(0, 3, n)]
        return grid(base + rng.integers(0, 4, n) * GRID)
    if kind == "negative-large":  # M = -S far right of -sqrt(rho): f large
        return grid(-(2.0 ** rng.uniform(16.0, 20.0, n)))
    if kind == "positive-large":  # M = -S far left: the literal f cancels
        return grid(2.0 ** rng.uniform(16.0, 20.0, n))
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------- bounds
def x_ref(M, rho):
    """Reference X = f(M) of the lower triangle of M (symmetric-eig semantics), with its eigenvalues."""
    lam, V = np.linalg.eigh(M, UPLO="L")
    return (V * f_stable(lam, rho)) @ V.T, lam


def x_bound(lam, M_fro, X_fro, rho, n):
    """||X_dev - X_ref||_F <= C n eps (L ||M||_F + ||X_ref||_F), L = f'(lambda_max) the Lipschitz constant of f on
    the spectrum (f convex and increasing; a Lipschitz f on R is Lipschitz with the same constant on symmetric
    matrices in the Frobenius norm): the backward error of the eigen-step carried through f, plus the rounding of
    V f V'."""
    L = float(fprime(np.max(lam), rho)) if len(lam) else 0.0
    return C * n * EPS * (L * M_fro + X_fro)


def logdet_bound(lam, M_fro, rho, n):
    """|(-log det X)_dev - (-log det X)_ref| <= sum_i |dl_i| / sqrt(l_i^2 + 4 rho) + C n eps sum_i |log f(l_i)|, with
    |dl_i| <= C n eps ||M||_F (d log f / dl = 1 / sqrt(l^2 + 4 rho)) and the second term the sum's rounding."""
    lam = np.asarray(lam, dtype=np.float64)
    dl = C * n * EPS * M_fro
    return float(np.sum(dl / np.sqrt(lam * lam + 4.0 * rho)) + C * n * EPS * np.sum(np.abs(np.log(f_stable(lam, rho)))))


def first_obj_bound(S, X_ref, lam, M_fro, rho, reg, n):
    """Bound on objevals[0] = trace(S X) - log det X + reg ||Z||_1 (Z = soft(X, reg / rho) at the first step),
    given ||X_dev - X_ref||_F <= x_bound: Cauchy-Schwarz for the trace, 1-Lipschitz soft threshold with
    ||.||_1 <= n ||.||_F, the n^2-term sums' rounding, and logdet_bound.

    The n^2-term rounding is the worst case, C n^2 eps sum|S .* X|: where the trace term is large it dominates, and the
    check then catches only gross errors in the objective (a missing or mis-signed term, det X overflowing).  Where
    the trace is small (rho = 2^20 with |s| <= 4: X ~ I / 2^10) the log-determinant term dominates, and
    test_first_x_update_logdet_alone holds -log det X to 4 n eps relative with S = 0."""
    bx = x_bound(lam, M_fro, np.linalg.norm(X_ref), rho, n)
    Z = np.sign(X_ref) * np.maximum(np.abs(X_ref) - reg / rho, 0.0)
    return (np.linalg.norm(S) * bx + reg * n * bx
            + C * n * n * EPS * (np.sum(np.abs(S * X_ref)) + reg * np.sum(np.abs(Z)))
            + logdet_bound(lam, M_fro, rho, n))


def cov_ref(D):
    """Two-pass cov(D) in long double: the centred Gram / (m - 1), and the centred |D - mu| for the bound."""
    Dl = np.asarray(D, dtype=np.longdouble)
    m = Dl.shape[0]
    Dc = Dl - Dl.sum(axis=0) / m
    return (Dc.T @ Dc) / (m - 1), np.abs(Dc)


def cov_bound(D, absDc):
    """Elementwise bound on the device's cov(D): C m eps (|D - mu|'|D - mu|) / (m - 1), the rounding of m-term dot
    products, plus the second-order effect of the computed column means, |dmu_i| |dmu_j| m / (m - 1), with
    |dmu| <= C (ceil(m / 256) + 9) eps mean|D| (one workgroup of 256 lanes: sequential adds, then a tree)."""
    D = np.asarray(D, dtype=np.float64)
    m = D.shape[0]
    A = np.asarray(absDc, dtype=np.float64)
    dmu = C * (math.ceil(m / 256) + 9) * EPS * np.mean(np.abs(D), axis=0)
    return C * m * EPS * (A.T @ A) / (m - 1) + np.outer(dmu, dmu) * m / (m - 1)


def ratio(err, bound):
    return float(err) / float(bound) if bound > 0 else (0.0 if err == 0 else math.inf)
