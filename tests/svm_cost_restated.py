"""The linear SVM with per-observation costs and the squared hinge restated in NumPy (a helper of test_svm_cost_host /
test_gpu_svm_cost, not a test):

    g(z) = C * sum_i c_i*phi(ell_i*z_i),   c_i = w_i*(ell_i > 0 ? cost_pos : cost_neg),   t_i = C*c_i/rho

under D*x = z, run by the oracle's unwrapped ADMM (unwrappedadmm.m:76-92 takes any separable z-prox).  With v = D*x + u
and s = ell.*v:

    hinge     phi(s) = max(1 - s, 0)       z = v + ell*max(min(1 - s, t), 0)
    sqhinge   phi(s) = max(1 - s, 0)^2     z = s >= 1 ? v : ell*(s + 2t)/(1 + 2t)
    logistic  phi(s) = log(1 + e^-s)       z = ell*root(s, t)         (logistic_restated.prox_root)
    01        phi(s) = [s < 1]             z = ell*y, y = s if s >= 1 or s < 1 - sqrt(2t), else 1

Every other loss string is the hinge prox with the 0-1 objective (linearsvm.m:154-158, 231-237)."""
import numpy as np

import logistic_restated as LR
from oracle import solvers_ref as S

EPS = float(np.finfo(np.float64).eps)
LOSSES = ("hinge", "sqhinge", "logistic", "01")


def cost_vector(ell, weights=None, classcost=(1.0, 1.0)):
    """c_i = w_i*(ell_i > 0 ? cost_pos : cost_neg); classcost may be 'balanced' = (m/(2 m_pos), m/(2 m_neg))"""
    ell = np.asarray(ell, dtype=np.float64).reshape(-1)
    if isinstance(classcost, str):
        assert classcost == "balanced"
        mp = int(np.sum(ell > 0))
        classcost = (ell.size / (2.0 * mp), ell.size / (2.0 * (ell.size - mp)))
    w = np.ones(ell.size) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    return w * np.where(ell > 0, float(classcost[0]), float(classcost[1]))


def prox(v, ell, t, loss, dtype=np.float64):
    """argmin_z 1/2*(z - v)^2 + t*phi(ell*z), element by element (t an array or a scalar); dtype = np.longdouble gives
    the value the fp64 results are measured against"""
    v = np.asarray(v, dtype=dtype)
    ell = np.asarray(ell, dtype=dtype)
    t = np.broadcast_to(np.asarray(t, dtype=dtype), v.shape)
    one, two = dtype(1), dtype(2)
    s = ell * v
    if loss == "logistic":
        return ell * LR.prox_root(s, t, dtype)
    if loss == "sqhinge":
        return np.where(s >= one, v, ell * ((s + two * t) / (one + two * t)))
    if loss == "01":
        return ell * np.where((s >= one) | (s < one - np.sqrt(two * t)), s, one)
    return v + ell * np.maximum(np.minimum(one - s, t), dtype(0))


def phi(s, loss, dtype=np.float64):
    s = np.asarray(s, dtype=dtype)
    h = np.maximum(dtype(1) - s, dtype(0))
    if loss == "hinge":
        return h
    if loss == "sqhinge":
        return h * h
    if loss == "logistic":
        return np.maximum(-s, dtype(0)) + np.log1p(np.exp(-np.abs(s)))
    return np.where(dtype(1) - s > 0, dtype(1), dtype(0))  # '01' and every other string


def objective(D, ell, C, cost, x, loss):
    """1/2*||x||^2 + C*sum(c.*phi(ell.*(D*x))): the convention of linearsvm.m:231-237 with the costs inside the sum"""
    return 0.5 * float(x @ x) + C * float(np.sum(cost * phi(ell * (D @ x), loss)))


def ratio(z, z_ld, v, t):
    """|z - z_ld| in units of eps*(|v| + t + 1)"""
    v = np.asarray(v, dtype=np.longdouble)
    t = np.asarray(t, dtype=np.longdouble)
    d = np.abs(np.asarray(z, dtype=np.longdouble) - np.asarray(z_ld, dtype=np.longdouble))
    return np.asarray(d / (EPS * (np.abs(v) + t + 1)), dtype=np.float64)


def run(D, ell, C, cost, loss, options=None, workers=1, maxiters=None):
    """the oracle's unwrapped ADMM with the restated prox as the caller's zming and the objective as options.obj.
    maxiters: unwrappedadmm.m:90 forces 1000; a shorter forced run enters the loop through the oracle's admm() with the
    operators and options unwrappedadmm.m:76-92 sets up (serial form only)"""
    options = dict(options or {})
    ell = np.asarray(ell, dtype=np.float64)
    cost = np.asarray(cost, dtype=np.float64)
    ploss = loss if loss in LOSSES else "hinge"
    if maxiters is not None:
        from oracle import admm_ref
        m = D.shape[0]
        Dplus = S.pinv_matlab(D)
        options.update(A=D, At=D.T, B=-1, nB=m, c=0, m=m, maxiters=int(maxiters), stopcond="both", nodualerror=1,
                       obj=lambda x, z: objective(D, ell, C, cost, x, loss))
        return admm_ref.admm(lambda _x, z, u, _rho: Dplus @ (z - u),
                             lambda x, _z, u, rho: prox(D @ x + u, ell, (C * cost) / rho, ploss), options)
    if options.get("parallel", "none") in ("both", "zming", "xminf"):  # linearsvm.m:170-205
        options["parallel"] = "both"
        starts = np.concatenate([[0], np.cumsum(S.slicemaker(options.get("slices", 0), workers, D.shape[0]))])

        def zming(x, _z, u, rho, k):
            lo, hi = int(starts[k]), int(starts[k + 1])
            return prox(D[lo:hi, :] @ x + u[lo:hi], ell[lo:hi], (C * cost[lo:hi]) / rho, ploss)
    else:
        def zming(x, _z, u, rho):
            return prox(D @ x + u, ell, (C * cost) / rho, ploss)
    options["obj"] = lambda x, z: objective(D, ell, C, cost, x, loss)
    return S.unwrappedadmm(zming, D, options, workers=workers)


# ---- the inputs of the element-update tests: s on and next to the kinks 1, 1 - t, 1 + 2t, plus random v
GRID_T = (0.0, 1e-12, 1.0, 1e6)


def element_inputs(length, t, costs, seed):
    """(v, ell, w) of `length` elements for the hinge, sqhinge and logistic element updates at t = C/rho: weights whose
    every 17th value is 0; the first twelve s = ell*v sit on and one ulp beside the element's own kinks 1, 1 - t_i,
    1 + 2 t_i (t_i = t*c_i) and 0, the rest is random, narrow and on the scale of t"""
    rng = np.random.default_rng(seed)
    ell = np.where(rng.random(length) < 0.5, 1.0, -1.0)
    w = rng.uniform(0.25, 4.0, length)
    w[::17] = 0.0
    ti = t * w * np.where(ell > 0, costs[0], costs[1])
    s = np.where(rng.random(length) < 0.5, rng.uniform(-3, 3, length), (1 + t) * rng.standard_normal(length))
    for j in range(min(12, length)):
        k = (1.0, 1.0 - ti[j], 1.0 + 2.0 * ti[j], 0.0)[j // 3]
        s[j] = (k, np.nextafter(k, np.inf), np.nextafter(k, -np.inf))[j % 3]
    return ell * s, ell, w


def element_inputs_01(length, t, costs, seed):
    """the same for the 0-1 update, CONSTRUCTED so that every s is at least 1e-6 away from both of its thresholds 1 and
    1 - sqrt(2 t_i) (t_i = t*c_i: they depend on the element's cost): each s is a threshold plus a signed offset of
    magnitude in [1e-6, 3], or the midpoint of a gap that is wide enough; no element is left out"""
    rng = np.random.default_rng(seed)
    ell = np.where(rng.random(length) < 0.5, 1.0, -1.0)
    w = rng.uniform(0.25, 4.0, length)
    w[::17] = 0.0
    ti = t * w * np.where(ell > 0, costs[0], costs[1])
    lo = 1.0 - np.sqrt(2.0 * ti)  # the lower threshold (= 1 where t_i = 0)
    off = 10.0 ** rng.uniform(-6, np.log10(3.0), length) * (1.0 + 1e-9) + 1e-6
    kind = rng.integers(0, 4, length)
    gap = 1.0 - lo
    s = np.where(kind == 0, 1.0 + off, np.where(kind == 1, lo - off * np.maximum(1.0, np.abs(lo)), 0.0))
    inside = kind >= 2
    # inside the band (lo, 1): where the gap is wide enough for a 2e-6 margin on both sides; else above 1
    mid = np.where(kind == 2, lo + 0.5 * gap, lo + np.minimum(0.25 * gap, 2e-6 + off))
    mid = np.where(gap > 8e-6 * np.maximum(1.0, np.abs(lo)), mid, 1.0 + off)
    s = np.where(inside, mid, s)
    assert np.all(np.abs(s - 1.0) >= 1e-6) and np.all(np.abs(s - lo) >= 1e-6)
    return ell * s, ell, w
