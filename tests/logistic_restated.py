"""The logistic loss of the linear SVM restated in NumPy (a helper of test_logistic_host / test_gpu_logistic, not a
test): g(z) = C*sum(log(1 + exp(-ell.*z))) under D*x = z, run by the oracle's unwrapped ADMM (unwrappedadmm.m:76-92
takes any separable z-prox).

The z-prox is z = ell.*s with s the root of phi(s) = (s - w) - t/(1 + e^s) in [w, w + t], w = ell.*(D*x + u),
t = C/rho.  phi' lies in [1, 1 + t/4], so |s - s*| <= |phi(s)|."""
import numpy as np

from oracle import solvers_ref as S

EPS = float(np.finfo(np.float64).eps)
PASSES = 200


def prox_root(w, t, dtype=np.float64, passes=PASSES):
    """Bracketed Newton on phi, run for a fixed generous number of passes (no stopping test).  A Newton step is taken
    when it lands inside the bracket and the previous step halved the bracket; otherwise the midpoint, so at least
    every other pass halves the bracket.  dtype = np.longdouble gives the value the fp64 results are measured against."""
    w = np.asarray(w, dtype=dtype)
    t = np.asarray(t, dtype=dtype)
    w, t = np.broadcast_arrays(w, t)
    one = dtype(1)
    lo, hi = w.copy(), w + t
    s = lo + (hi - lo) / 2
    wprev = np.full(w.shape, np.inf, dtype=dtype)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for _ in range(passes):
            e = np.exp(-np.abs(s))
            sig = np.where(s >= 0, e / (one + e), one / (one + e))  # 1/(1 + e^s) from e^-|s|
            phi = (s - w) - t * sig
            dphi = one + t * e / ((one + e) * (one + e))
            lo = np.where(phi < 0, s, lo)
            hi = np.where(phi > 0, s, hi)
            sn = s - phi / dphi
            wid = hi - lo
            bisect = ~((sn >= lo) & (sn <= hi)) | (wid > wprev / 2)
            wprev = np.where(bisect, np.inf, wid)
            s = np.where(bisect, lo + (hi - lo) / 2, sn)
    return s


def ratio(s, s_ld, w, t):
    """|s - s_ld| in units of eps*(|w| + t + 1)"""
    w = np.asarray(w, dtype=np.longdouble)
    t = np.asarray(t, dtype=np.longdouble)
    d = np.abs(np.asarray(s, dtype=np.longdouble) - np.asarray(s_ld, dtype=np.longdouble))
    return np.asarray(d / (EPS * (np.abs(w) + t + 1)), dtype=np.float64)


# the grid of the element-update tests, and the random pairs that go with it
GRID_W = (800.0, -800.0, 40.0, -40.0, 3.0, -3.0, 1e-8, -1e-8, 0.0, -1e-300)
GRID_T = (0.0, 1e-12, 1.0, 1e6)


def grid_pairs():
    W, T = np.meshgrid(np.array(GRID_W), np.array(GRID_T), indexing="ij")
    return W.ravel(), T.ravel()


def random_pairs(count=4000, seed=5):
    rng = np.random.default_rng(seed)
    k = count // 4
    w = np.concatenate([rng.uniform(-50, 50, k), 1e3 * rng.standard_normal(k), rng.uniform(-1e4, 1e4, k)])
    t = np.concatenate([10.0 ** rng.uniform(-12, 6, k), 10.0 ** rng.uniform(-3, 6, k), 10.0 ** rng.uniform(-2, 6, k)])
    tb = 10.0 ** rng.uniform(-2, 6, count - 3 * k)  # the band where the root is near 0: w + t/2 ~ 0
    return np.concatenate([w, -tb / 2 + rng.standard_normal(tb.size)]), np.concatenate([t, tb])


def prox(v, ell, t, dtype=np.float64):
    return np.asarray(ell, dtype=dtype) * prox_root(np.asarray(ell, dtype=dtype) * np.asarray(v, dtype=dtype), t, dtype)


def loss_sum(q):
    """sum log(1 + exp(-q))"""
    return float(np.sum(np.logaddexp(0.0, -np.asarray(q, dtype=np.float64))))


def objective(D, ell, C, x):
    """1/2*||x||^2 + C*sum(log(1 + exp(-ell.*(D*x)))): the convention of linearsvm.m:231-237"""
    return 0.5 * float(x @ x) + C * loss_sum(ell * (D @ x))


def run(D, ell, C, options, workers=1, maxiters=None):
    """the oracle's unwrapped ADMM with the restated prox as the caller's zming and the objective as options.obj.
    maxiters: unwrappedadmm.m:90 forces 1000; a shorter forced run enters the loop through the oracle's admm() with the
    operators and options unwrappedadmm.m:76-92 sets up (serial form only)"""
    options = dict(options or {})
    ell = np.asarray(ell, dtype=np.float64)
    if maxiters is not None:
        from oracle import admm_ref
        m = D.shape[0]
        Dplus = S.pinv_matlab(D)
        options.update(A=D, At=D.T, B=-1, nB=m, c=0, m=m, maxiters=int(maxiters), stopcond="both", nodualerror=1,
                       obj=lambda x, z: objective(D, ell, C, x))
        return admm_ref.admm(lambda _x, z, u, _rho: Dplus @ (z - u),
                             lambda x, _z, u, rho: prox(D @ x + u, ell, C / rho), options)
    if options.get("parallel", "none") in ("both", "zming", "xminf"):  # linearsvm.m:170-205
        options["parallel"] = "both"
        starts = np.concatenate([[0], np.cumsum(S.slicemaker(options.get("slices", 0), workers, D.shape[0]))])

        def zming(x, _z, u, rho, k):
            lo, hi = int(starts[k]), int(starts[k + 1])
            return prox(D[lo:hi, :] @ x + u[lo:hi], ell[lo:hi], C / rho)
    else:
        def zming(x, _z, u, rho):
            return prox(D @ x + u, ell, C / rho)
    options["obj"] = lambda x, z: objective(D, ell, C, x)
    return S.unwrappedadmm(zming, D, options, workers=workers)
