"""The loss family of the LAD and Huber engines restated in NumPy (a helper of test_loss_host / test_gpu_loss, not a
test):

    minimise g(z) subject to D*x - z = s,   g(z) = sum_i w_i*phi(z_i),
    lad:      phi(z) = a*max(z - eps, 0) + b*max(-z - eps, 0)
    huberfit: phi(z) = (z >= 0 ? a : b)*H_delta(z),  H_delta(z) = z^2/2 for |z| <= delta, delta*|z| - delta^2/2 beyond

The oracle's admm runs with the x-update of oracle.proxops_ref.getproxops('LAD' | 'HuberFit', ...) and, as the caller's
zming, prox_{g/rho}(v), v = D*x + u - s (the relaxed D*x when relax != 1), with t_a = w_i*a/rho, t_b = w_i*b/rho:

    lad:      z = v - t_a (v > eps + t_a), eps (v >= eps), v (v > -eps), -eps (v >= -eps - t_b), v + t_b otherwise
    huberfit: z = v - clamp(alpha*v/(alpha + rho), lo, hi), alpha = w_i*a and (lo, hi) = (0, alpha*delta/rho) for v >= 0,
              alpha = w_i*b and (lo, hi) = (-alpha*delta/rho, 0) for v < 0

test_loss_host checks the subgradient condition of w*phi(z) + rho/2*(z - v)^2 instead of trusting this."""
import numpy as np
import scipy.linalg as sla

from oracle import admm_ref
from oracle.proxops_ref import getproxops

EPS = float(np.finfo(np.float64).eps)


class Loss:
    """one member of the family on a 'lad' or 'huberfit' engine"""

    def __init__(self, kind, weights=None, slopes=(1.0, 1.0), epsilon=0.0, delta=1.0):
        assert kind in ("lad", "huberfit")
        self.kind = kind
        self.w = None if weights is None else np.asarray(weights, dtype=np.float64)
        self.a, self.b = float(slopes[0]), float(slopes[1])
        self.eps, self.delta = float(epsilon), float(delta)

    def options(self):
        """the fields as ap.lad / ap.huberfit read them from options"""
        o = {}
        if self.w is not None:
            o["weights"] = self.w
        if (self.a, self.b) != (1.0, 1.0):
            o["slopes"] = (self.a, self.b)
        if self.eps:
            o["epsilon"] = self.eps
        if self.delta != 1.0:
            o["delta"] = self.delta
        return o


def prox(v, loss, rho, dtype=np.float64):
    """prox_{g/rho}(v); dtype = np.longdouble gives the value fp64 results are measured against"""
    v = np.asarray(v, dtype=dtype)
    w = np.ones(v.size, dtype=dtype) if loss.w is None else loss.w.astype(dtype)
    rho, a, b = dtype(rho), dtype(loss.a), dtype(loss.b)
    if loss.kind == "huberfit":
        delta = dtype(loss.delta)
        pos = v >= 0
        alpha = w * np.where(pos, a, b)
        q = (alpha * v) / (alpha + rho)
        lim = (alpha * delta) / rho
        s = np.where(pos, np.minimum(np.maximum(q, 0), lim), np.maximum(np.minimum(q, 0), -lim))
        return v - s
    eps = dtype(loss.eps)
    ta, tb = (w * a) / rho, (w * b) / rho
    return np.where(v > eps + ta, v - ta,
                    np.where(v >= eps, eps + 0 * v, np.where(v > -eps, v, np.where(v >= -eps - tb, -eps + 0 * v, v + tb))))


def phi(z, loss):
    """phi(z_i) per element (without the weights)"""
    z = np.asarray(z)
    if loss.kind == "huberfit":
        az = np.abs(z)
        h = np.where(az <= loss.delta, 0.5 * z * z, loss.delta * az - 0.5 * loss.delta ** 2)
        return np.where(z >= 0, loss.a, loss.b) * h
    return loss.a * np.maximum(z - loss.eps, 0.0) + loss.b * np.maximum(-z - loss.eps, 0.0)


def g_of(z, loss):
    w = 1.0 if loss.w is None else loss.w
    return float(np.sum(w * phi(z, loss)))


def dphi_interval(z, loss):
    """the subdifferential of phi at every z_i as an interval [lo, hi]"""
    z = np.asarray(z, dtype=np.float64)
    if loss.kind == "huberfit":
        d = np.clip(z, -loss.delta, loss.delta)
        lo = np.where(z > 0, loss.a * d, np.where(z < 0, loss.b * d, 0.0))
        return lo, lo.copy()
    e, a, b = loss.eps, loss.a, loss.b
    lo = np.where(z > e, a, np.where(z >= -e, 0.0, -b))
    hi = np.where(z >= e, a, np.where(z > -e, 0.0, -b))
    if e == 0.0:  # the kink at 0 joins both sides
        lo = np.where(z == 0, -b, lo)
        hi = np.where(z == 0, a, hi)
    else:
        lo = np.where(z == -e, -b, lo)
        hi = np.where(z == -e, 0.0, hi)
        lo = np.where(z == e, 0.0, lo)
    return lo, hi


def run(kind, D, s, loss, options=None):
    """lad.m:124-148 / huberfit.m:156-180 with this z-update as the caller's zming (as penalty_restated.run)"""
    assert kind == loss.kind
    options = dict(options or {})
    m, n = D.shape
    args = dict(D=D, s=s, R=sla.cholesky(D.T @ D, lower=True))
    relaxed = options.get("relax", 1) != 1
    if relaxed:
        args["userelax"] = 1
    minx, _, _ = getproxops("LAD" if kind == "lad" else "HuberFit", args)
    if relaxed:
        zming = lambda dxhat, _z, u, r: prox(dxhat + u - s, loss, r)
    else:
        zming = lambda x, _z, u, r: prox(D @ x + u - s, loss, r)
    options.update(A=D, B=-1, c=s, m=m, nA=n, nB=m)
    options["obj"] = lambda x, z: g_of(z, loss)
    return admm_ref.admm(minx, zming, options)


def bound_ratio(v, got, exact, loss, rho):
    """worst |got_i - exact_i| / (12*eps*(|v_i| + t_a + t_b + epsilon)) over the elements: penalty_restated.bound_ratio's
    constant for a chain no shorter than these (product, quotient, sum, comparison, difference)"""
    n = len(v)
    w = np.ones(n) if loss.w is None else loss.w
    size = np.abs(v).astype(np.longdouble) + (w * loss.a / rho + w * loss.b / rho + loss.eps).astype(np.longdouble)
    bound = np.longdouble(12 * EPS) * size
    d = np.abs(np.asarray(got, dtype=np.longdouble) - exact)
    assert np.all(d[bound == 0] == 0)
    nz = bound > 0
    return float(np.max(d[nz] / bound[nz])) if nz.any() else 0.0


def breakpoint_vector(loss, rho, n=1000, seed=21):
    """v that spans every branch of the prox and sits exactly on every breakpoint (of every distinct weight among the
    first elements): the operator test's input"""
    rng = np.random.default_rng(seed)
    w = np.ones(n) if loss.w is None else loss.w
    if loss.kind == "lad":
        scale = loss.eps + (loss.a + loss.b) * float(np.max(w)) / rho
    else:
        scale = loss.delta * (1.0 + (loss.a + loss.b) * float(np.max(w)) / rho)
    v = rng.uniform(-2.5 * scale, 2.5 * scale, n)
    k = min(n // 8, 100)
    for j in range(k):  # element j sits on a breakpoint of its own weight
        if loss.kind == "lad":
            ta, tb = (w[j] * loss.a) / rho, (w[j] * loss.b) / rho
            pts = (loss.eps + ta, loss.eps, -loss.eps, -loss.eps - tb, 0.0)
        else:
            pa, pb = w[j] * loss.a, w[j] * loss.b
            pts = (loss.delta * (pa + rho) / rho, -loss.delta * (pb + rho) / rho, 0.0, loss.delta, -loss.delta)
        v[j] = pts[j % len(pts)]
    return v


# ------------------------------------------------------------------------------------ the fixtures of the tests
MEMBERS = ("quantile", "svr", "huber")


def member(name, m, seed=0):
    """quantile with weights; SVR (a dead zone); Huber with delta = 0.5, a != b and weights.  Weights: uniform in
    [0.5, 2] with one zero (an observation that does not count)."""
    rng = np.random.default_rng(seed + 700)
    w = rng.uniform(0.5, 2.0, m)
    w[min(5, m - 1)] = 0.0
    if name == "quantile":
        return Loss("lad", weights=w, slopes=(0.8, 0.2))
    if name == "svr":
        return Loss("lad", epsilon=0.3)
    if name == "huber":
        return Loss("huberfit", weights=w, slopes=(1.5, 0.5), delta=0.5)
    raise ValueError(name)


def regression(synth, rows, cols, seed):
    """synth.quantile_problem: an intercept, standard normal regressors, heteroscedastic noise"""
    p = synth.quantile_problem(seed, rows, cols)
    return p["D"], p["s"]
