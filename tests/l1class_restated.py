"""The sparse linear classifier restated in NumPy (a helper of test_l1class_host / test_gpu_l1class, not
a test): per fit

    minimise C*sum_i c_i*phi(ell_i*(D*x)_i) + lambda*sum_j w_j*|x_j| + mu/2*||x||^2   [x >= 0 when nonnegative]

run by the oracle's admm (oracle.admm_ref.admm) with A = [D; I_n], B = -1, c = 0, z = [z1 (m); z2 (n)]:

    xminf   x = (D'D + I)^-1 (D'(z1 - u1) + (z2 - u2)), a SciPy Cholesky of D'D + I
    zming   z1 = svm_cost_restated.prox(D*x + u1, ell, C*c/rho, loss),  z2 = penalty_restated.prox(x + u2, ...)
    obj     the expression above with the loss at D*x and the penalty at z2

``kkt`` returns the worst violation of the optimality conditions, which is how test_l1class_host trusts all of it."""
import numpy as np
import scipy.linalg as sla

import penalty_restated as P
import svm_cost_restated as SC
from oracle import admm_ref

SLOPE0 = dict(logistic=0.5, hinge=1.0, sqhinge=2.0)  # |phi'(0)|


class Fit:
    """one fit: the loss, lambda, the penalty's members and the costs"""

    def __init__(self, loss="logistic", lam=0.1, ridge=0.0, nonnegative=0, l1weights=None, weights=None,
                 classcost=(1.0, 1.0), C=1.0):
        self.loss, self.lam, self.C = loss, float(lam), float(C)
        self.pen = P.Penalty(l1weights=l1weights, ridge=ridge, nonnegative=nonnegative)
        self.weights, self.classcost = weights, classcost

    def cost(self, ell):
        return SC.cost_vector(ell, self.weights, self.classcost)

    def options(self):
        """the fields as ap.l1classifier reads them from options"""
        o = dict(self.pen.options(), lossfunction=self.loss, C=self.C)
        if self.weights is not None:
            o["weights"] = self.weights
        if self.classcost != (1.0, 1.0):
            o["classcost"] = self.classcost
        return o


def dphi(s, loss):
    """phi'(s); the hinge's subgradient at the kink is taken as -1 (kkt is called on smooth losses)"""
    if loss == "logistic":
        return -1.0 / (1.0 + np.exp(s))
    if loss == "sqhinge":
        return -2.0 * np.maximum(1.0 - s, 0.0)
    return np.where(s < 1.0, -1.0, 0.0)


def objective(D, ell, fit, x, z2):
    w = 1.0 if fit.pen.w is None else fit.pen.w
    return (fit.C * float(np.sum(fit.cost(ell) * SC.phi(ell * (D @ x), fit.loss))) + fit.lam * float(np.sum(w * np.abs(z2)))
            + 0.5 * fit.pen.ridge * float(z2 @ z2))


def lambda_max(D, ell, fit):
    """C*|phi'(0)|*max over w_j > 0 of |sum_i c_i*ell_i*D_ij| / w_j"""
    g = np.abs(D.T @ (fit.cost(ell) * ell))
    if fit.pen.w is not None:
        g = g[fit.pen.w > 0] / fit.pen.w[fit.pen.w > 0]
    return fit.C * SLOPE0[fit.loss] * float(g.max())


def run(D, ell, fit, options=None):
    """the oracle's plain loop on the stacked problem; options: rho, abstol, reltol, maxiters, domaxiters, objevals,
    nodualerror, z0, u0 (m + n entries each)"""
    options = dict(options or {})
    m, n = D.shape
    ell = np.asarray(ell, dtype=np.float64).reshape(-1)
    cost = fit.cost(ell)
    F = sla.cho_factor(D.T @ D + np.eye(n), lower=True)
    A = np.vstack([D, np.eye(n)])

    def xminf(_x, z, u, _rho):
        t = z - u
        return sla.cho_solve(F, D.T @ t[:m] + t[m:])

    def zming(x, _z, u, rho):
        z1 = SC.prox(D @ x + u[:m], ell, (fit.C * cost) / rho, fit.loss)
        z2 = P.prox(x + u[m:], fit.pen, fit.lam / rho, 0.0, rho)
        return np.concatenate([z1, z2])

    options.update(A=A, B=-1, c=0, m=m + n, nB=m + n, stopcond="standard",
                   obj=lambda x, z: objective(D, ell, fit, x, z[m:]))
    options.setdefault("x0", np.zeros(n))
    return admm_ref.admm(xminf, zming, options)


def kkt(D, ell, fit, x):
    """the worst violation of  |g_j + mu*x_j| <= lambda*w_j where x_j = 0  and  g_j + mu*x_j = -lambda*w_j*sign(x_j)
    elsewhere (one-sided under nonnegative: g_j + mu*x_j >= -lambda*w_j where x_j = 0), g = C*D'(c.*ell.*phi'(ell.*D*x))"""
    ell = np.asarray(ell, dtype=np.float64).reshape(-1)
    n = D.shape[1]
    w = np.ones(n) if fit.pen.w is None else fit.pen.w
    g = fit.C * (D.T @ (fit.cost(ell) * ell * dphi(ell * (D @ x), fit.loss))) + fit.pen.ridge * x
    lw = fit.lam * w
    zero = x == 0
    v = np.zeros(n)
    if fit.pen.nonnegative:
        v[zero] = np.maximum(-lw[zero] - g[zero], 0.0)
        v[~zero] = np.where(x[~zero] > 0, np.abs(g[~zero] + lw[~zero]), np.inf)
    else:
        v[zero] = np.maximum(np.abs(g[zero]) - lw[zero], 0.0)
        v[~zero] = np.abs(g[~zero] + lw[~zero] * np.sign(x[~zero]))
    return float(v.max())


def problem(shape, K=1, seed=0):
    """dict(D, ELL (m x K), z0, u0 ((m + n) x K)): unit columns, labels from a sparse truth per fit plus noise, small
    random starts shared by the device run and the restated one"""
    m, n = shape
    rng = np.random.default_rng(1000 * m + n + seed)
    D = rng.standard_normal((m, n))
    D /= np.linalg.norm(D, axis=0)
    ELL = np.empty((m, K), order="F")
    for k in range(K):
        truth = np.where(rng.random(n) < 0.1, rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 3.0, n), 0.0)
        truth[k % n] = 2.0
        ELL[:, k] = np.where(D @ truth + 0.1 * rng.standard_normal(m) >= 0, 1.0, -1.0)
    z0, u0 = (np.asfortranarray(0.1 * rng.standard_normal((m + n, K))) for _ in range(2))
    return dict(D=np.asfortranarray(D), ELL=ELL, z0=z0, u0=u0)
