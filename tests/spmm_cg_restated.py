"""The lock-step conjugate gradients of the sparse multi-fit solvers, ONE solve of one right-hand side, restated in NumPy
(a helper of test_spmm_cg_host / test_gpu_spmm_cg, not a test): the recurrence of
sparse_lasso_restated.CgShift on (D'D + shift*I) x = y with its four exits explicit -- ||r|| <= tol*||y||, maxit, a zero
right-hand side (x = 0) and p.q = 0 (nothing divided or updated) -- in float64, or in longdouble as the high-precision
reference of the same operation.

Also the cases of the two test files.  A case is a matrix of sparse_cases.problem (row 3 dense, row 5 and column 7 empty),
a shift, a tolerance, a cap and one (kind, seed) per fit; column k of a case with K > 1 fits is scaled by
10^(-3 + 6k/(K-1)), six orders of magnitude over the case, so that no relative measure is carried by the largest column.

The seeds.  A device that adds in another order may only be asked for the restatement's iteration count where the stop
test cannot flip: sqrt(rs) / (tol*||y||) outside [0.5, 2] at the last inner iteration and at the one before it (guard()),
and where the count belongs to the operation and not to its rounding: the longdouble restatement, left to its own stop
test, passes guard() too, ends with the same counters and agrees on the deciding ratios within a factor 2 (stable()).  Most right-hand sides cross the tolerance more
slowly than that, so every seed of a "range" fit below is the smallest one, walking up from 0 and skipping those of the
fits in front of it, that passes stable() at its place in its case; test_spmm_cg_host checks every one of them again."""
from collections import namedtuple

import numpy as np

from sparse_cases import problem

# the largest relative gap in x (relative to ||x||_inf of the fit) between the float64 and the longdouble restatement at
# equal iteration count over every fit of CASES, as test_spmm_cg_host.test_float64_against_longdouble_measures_the_bounds
# printed it; the device's bound is 10x this (the project's margin for its summation order inside the products, as
# sparse_lasso_restated.PARITY_BOUND)
MEASURED_X_GAP = 2.2e-10  # 2.169e-10: "A65 shift 0 generic" fit 0, 48 iterations at cond 390
# the largest | ||r_recurrence|| - ||r_true|| | / ||y|| of the float64 restatement over the same fits, r_true in
# longdouble from the float64 x
MEASURED_DRIFT = 2.2e-15  # 2.197e-15: "n = 31 shift 0" fit 5, 38 iterations
# two vectors whose norms agree need not agree: the largest ||r_recurrence - r_true|| / ||y|| over the same fits, for the
# comparison of the returned R with the true residual entry by entry
MEASURED_R_GAP = 1.2e-14  # 1.108e-14: "n = 32 shift 0" fit 8, 41 iterations
X_BOUND = 10.0 * MEASURED_X_GAP
DRIFT_BOUND = 10.0 * MEASURED_DRIFT
R_BOUND = 10.0 * MEASURED_R_GAP
assert X_BOUND <= 1e-6  # never looser than the project's parity definition

A65 = (257, 65, 0.03)
FAT = (80, 200, 0.10)
WIDE = (60, 8300, 0.02)  # more than 32 * 256 coefficients: a workgroup of an elementwise kernel takes a second row block
TINY = {1: (40, 1, 0.5), 31: (40, 31, 0.3), 32: (40, 32, 0.3), 33: (40, 33, 0.3)}  # n at and around one row block
EMPTY_COLUMN = 7
FEW = 6


def cg(D, y, x0, shift, tol, maxit, dtype=np.float64):
    """dict(x, r, iters, capped, brk, zero, ratios): x0 None starts from 0 with r = y (the first solve of a run), else
    from x0 with r = y - (D'(D x0) + shift*x0).  ratios: sqrt(rs) / (tol*||y||) at the start and behind every inner
    iteration that updated x (empty for a zero right-hand side)"""
    D = np.asarray(D, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    shift, tol = dtype(shift), dtype(tol)
    n = D.shape[1]
    if x0 is None:
        x, r = np.zeros(n, dtype=dtype), y.copy()
    else:
        x = np.asarray(x0, dtype=dtype).copy()
        r = y - (D.T @ (D @ x) + shift * x)
    yy, rs = y @ y, r @ r
    if yy == 0.0:
        return dict(x=np.zeros(n, dtype=dtype), r=r, iters=0, capped=0, brk=0, zero=1, ratios=[])
    ynorm = np.sqrt(yy)
    ratio = lambda: float(np.sqrt(rs) / (tol * ynorm)) if tol > 0 else np.inf
    ratios = [ratio()]
    p = r.copy()
    it, brk, converged = 0, 0, np.sqrt(rs) <= tol * ynorm
    while not converged and it < maxit:
        q = D.T @ (D @ p) + shift * p
        pq = p @ q
        it += 1
        if pq == 0.0:
            brk = 1
            break
        alpha = rs / pq
        x = x + alpha * p
        r = r - alpha * q
        rsn = r @ r
        p = r + (rsn / rs) * p
        rs = rsn
        ratios.append(ratio())
        converged = np.sqrt(rs) <= tol * ynorm
    return dict(x=x, r=r, iters=it, capped=0 if converged else 1, brk=brk, zero=0, ratios=ratios)


def true_residual(D, y, x, shift):
    """y - (D'(D x) + shift*x) in longdouble"""
    D = np.asarray(D, dtype=np.longdouble)
    x = np.asarray(x, dtype=np.longdouble)
    return np.asarray(y, dtype=np.longdouble) - (D.T @ (D @ x) + np.longdouble(shift) * x)


def guard(res):
    """the stop test of this fit cannot flip under another summation order: the ratios of the last inner iteration and of
    the one before it (the start, where there is none) lie outside [0.5, 2].  A zero right-hand side and the p.q = 0 exit
    are decided by exact zeros and pass"""
    if res["zero"] or res["brk"]:
        return True
    return all(not 0.5 <= v <= 2.0 for v in res["ratios"][-2:])


def stable(f64, ld):
    """guard() for the float64 run and for the longdouble run under its own stop test, the same counters, and the two
    deciding ratios of one run within a factor 2 of the other's, or both below 1e-3: a residual that is what rounding
    left behind an exact termination has a norm that belongs to the rounding, and decides nothing only where it stays a
    thousand times below the tolerance"""
    if not (guard(f64) and guard(ld) and all(f64[f] == ld[f] for f in ("iters", "capped", "brk", "zero"))):
        return False
    return all(0.5 * b <= a <= 2.0 * b or max(a, b) <= 1e-3 for a, b in zip(f64["ratios"][-2:], ld["ratios"][-2:]))


# ---- the cases
# A fit is (kind, seed):
#   "range"  y = D's, s standard normal from the seed: in range(D'), as every right-hand side of a solver with shift = 0;
#            behind a warm start x0 = 0.01 * D't, t from the seed + 50000
#   "few"    y = D's with s random in the span of FEW left singular vectors of D: CG ends after FEW iterations, the
#            residual falling by orders of magnitude in the last one; behind a warm start x0 = 0.01 * D't, t in the same
#            span.  For 80 x 200 with shift 0 and 1 and 257 x 65 with shift 0: no seed up to 5000 of a "range" fit there
#            passes stable(), the residual crosses tol by less than a factor 4 per iteration
#   "e7"     y = seed * e_7, the unit vector of the empty column (an integer multiple, never scaled): D p = 0, so without
#            a shift p.q = 0, and with one x = y / shift in one iteration; behind a warm start x0 = 0.75 * e_7
#   "zero"   y = 0; behind a warm start x0 = D't, t from the seed
#   "copy"   the fit `seed` of the same case once more, bit for bit
# warm: None (from x = 0, the first solve of a run), "own" (the x0 of the kinds above), or the name of the case whose
# float64 solution is x0.  counts: the iteration count is compared (every fit passes guard())
Case = namedtuple("Case", "shape shift tol maxit warm fits counts")


def _fits(seeds, **other):
    """"range" fits from the seeds, with the fits of `other` (fit=(kind, seed)) put in at their places"""
    fits = [("range", s) for s in seeds]
    for k, f in sorted(other.items()):
        fits.insert(int(k[1:]), f)
    return tuple(fits)


SEEDS = {
    "A65 shift 0 generic": (47, 38, 18),
    "A65 shift 1": (5, 6, 12, 15, 16, 19, 22, 30, 31, 34, 35),
    "A65 shift 2.5": (3, 34, 9, 5, 12, 4, 6, 16, 15, 28, 11, 7, 27, 22, 31, 39, 35, 46, 37, 49, 38),
    "FAT shift 2.5": (3, 13, 15, 19, 22, 30, 41, 43, 46, 59),
    "n = 31 shift 1": (2, 9, 23, 27, 34, 38, 44, 46, 47, 49, 54),
    "n = 32 shift 1": (1, 16, 18, 23, 25, 28, 51, 53, 64, 66, 69),
    "n = 33 shift 1": (21, 22, 24, 42, 48, 49, 51, 53, 55, 58, 60),
    "WIDE shift 0": (0, 3, 4),
    "WIDE shift 2.5": (0, 5, 6),
    "e7 shift 2": (8, 9),
    "zero": (5, 6),
    "zero warm": (5, 6),
    "mixed": (0, 11, 33, 81, 168, 187, 191, 211, 214),
}  # (a case that is not listed: 0, 1, 2, ...)


def _case(name, shape, shift, tol, maxit, warm, K, counts=True, **other):
    seeds = SEEDS.get(name, tuple(range(K - len(other))))
    assert len(seeds) == K - len(other), name
    return Case(shape, shift, tol, maxit, warm, _fits(seeds, **other), counts)


def _cases():
    c = {}
    # iterate parity: both instantiations (shift = 0 and not) on both matrices, every K of {1, 3, 10, 11, 21}
    c["A65 shift 0"] = _case("A65 shift 0", A65, 0.0, 1e-10, 200, None, 3, k0=("few", 0), k1=("few", 2), k2=("few", 4))
    # ordinary right-hand sides without a shift: 45 to 49 iterations at cond 390, where rounding alone moves the count (the
    # float64 restatement stops at 48, the longdouble one at 46), so no count is compared
    c["A65 shift 0 generic"] = _case("A65 shift 0 generic", A65, 0.0, 1e-10, 200, None, 3, counts=False)
    c["A65 shift 1"] = _case("A65 shift 1", A65, 1.0, 1e-10, 200, None, 11)
    c["A65 shift 2.5"] = _case("A65 shift 2.5", A65, 2.5, 1e-10, 200, None, 21)
    c["FAT shift 0"] = _case("FAT shift 0", FAT, 0.0, 1e-10, 200, None, 1, k0=("few", 0))
    c["FAT shift 1"] = _case("FAT shift 1", FAT, 1.0, 1e-10, 200, None, 3, k0=("few", 0), k1=("few", 2), k2=("few", 4))
    c["FAT shift 2.5"] = _case("FAT shift 2.5", FAT, 2.5, 1e-10, 200, None, 10)
    # row-block edges
    for n, shape in TINY.items():
        for shift in (0.0, 1.0):
            name = f"n = {n} shift {shift:g}"
            # (without a shift no seed up to 5000 passes stable() on these matrices, of either kind: no count is compared)
            c[name] = _case(name, shape, shift, 1e-10, 200, None, 11, counts=shift != 0.0 or n == 1)
    c["WIDE shift 0"] = _case("WIDE shift 0", WIDE, 0.0, 1e-10, 200, None, 3)
    c["WIDE shift 2.5"] = _case("WIDE shift 2.5", WIDE, 2.5, 1e-10, 200, None, 3)
    # independence of neighbours: "A65 shift 2.5" with fit 0 again at 10 and 20
    c["same three"] = c["A65 shift 2.5"]._replace(
        fits=tuple(("copy", 0) if k in (10, 20) else f for k, f in enumerate(c["A65 shift 2.5"].fits)))
    # the exit without a division, in the middle fit
    c["brk"] = _case("brk", A65, 0.0, 1e-10, 200, None, 3, k0=("few", 6), k1=("e7", 1), k2=("few", 8))
    c["brk warm"] = _case("brk warm", A65, 0.0, 1e-10, 200, "own", 3, k0=("few", 6), k1=("e7", 1), k2=("few", 8))
    c["e7 shift 2"] = _case("e7 shift 2", A65, 2.0, 1e-10, 200, None, 3, k1=("e7", 1))
    # a zero right-hand side, in the middle fit
    c["zero"] = _case("zero", A65, 1.0, 1e-10, 200, None, 3, k1=("zero", 7))
    c["zero warm"] = _case("zero warm", A65, 1.0, 1e-10, 200, "own", 3, k1=("zero", 7))
    # a converged warm start: the x of "tight" under a looser tolerance
    c["tight"] = _case("tight", A65, 1.0, 1e-13, 200, None, 11, counts=False)
    c["converged"] = c["tight"]._replace(tol=1e-8, warm="tight", counts=True)
    # mixed finish inside a chunk: fit 0 ends after one iteration, the others after more than 20
    c["mixed"] = _case("mixed", A65, 0.5, 1e-12, 200, None, 10, k0=("e7", 3))
    # the cap: the restatement needs 13 iterations.  (An iterate in the middle of a solve is far more sensitive to
    # rounding than the solution: with shift 1 the float64 and the longdouble x of iteration 9 are 3e-8 apart)
    for maxit in (1, 3, 5, 9):
        c[f"maxit {maxit}"] = _case("maxit", A65, 2.5, 1e-10, maxit, None, 3)
    return c


CASES = _cases()
_CACHE = {}


def matrix(ap, shape):
    key = ("A", tuple(shape))
    if key not in _CACHE:
        _CACHE[key] = problem(ap, *shape, seed=1)["A"]
    return _CACHE[key]


def left_vectors(A):
    key = ("U", A.shape)
    if key not in _CACHE:
        _CACHE[key] = np.linalg.svd(A, full_matrices=False)[0]  # (singular values descending: the first rank columns)
    return _CACHE[key]


def scale(K, k):
    return 1.0 if K == 1 else 10.0 ** (-3.0 + 6.0 * k / (K - 1))


def column(A, case, k):
    """(y, x0 | None) of fit k; a warm start from another case's solution is put in by inputs()"""
    kind, seed = case.fits[k]
    m, n = A.shape
    own = case.warm == "own"
    if kind == "copy":
        return column(A, case, seed)
    if kind == "e7":
        e = np.zeros(n)
        e[EMPTY_COLUMN] = 1.0
        return float(seed) * e, (0.75 * e if own else None)
    sc = scale(len(case.fits), k)
    if kind == "zero":
        return np.zeros(n), (sc * (A.T @ np.random.default_rng(seed).standard_normal(m)) if own else None)
    if kind == "few":
        U, idx = left_vectors(A), np.random.default_rng(seed).choice(np.linalg.matrix_rank(A), FEW, replace=False)
        coeffs = np.random.default_rng(seed + 1).standard_normal((FEW, 2))
        return sc * (A.T @ (U[:, idx] @ coeffs[:, 0])), (sc * 0.01 * (A.T @ (U[:, idx] @ coeffs[:, 1])) if own else None)
    assert kind == "range", kind
    y = sc * (A.T @ np.random.default_rng(seed).standard_normal(m))
    return y, (sc * 0.01 * (A.T @ np.random.default_rng(seed + 50000).standard_normal(m)) if own else None)


def inputs(ap, name):
    """dict(case, A dense, D csc_matrix, Y n x K, X0 n x K | None), computed once"""
    import scipy.sparse as sp
    key = ("in", name)
    if key not in _CACHE:
        case = CASES[name]
        A = matrix(ap, case.shape)
        cols = [column(A, case, k) for k in range(len(case.fits))]
        Y = np.asfortranarray(np.column_stack([y for y, _ in cols]))
        X0 = None
        if case.warm == "own":
            X0 = np.asfortranarray(np.column_stack([x0 for _, x0 in cols]))
        elif case.warm is not None:
            X0 = np.asfortranarray(np.column_stack([r["x"] for r in restated(ap, case.warm, np.float64)]))
        _CACHE[key] = dict(case=case, A=A, D=sp.csc_matrix(A), Y=Y, X0=X0)
    return _CACHE[key]


def restated(ap, name, dtype, iters=None):
    """the restatement of every fit of a case, computed once and never changed; iters: one forced count per fit in place
    of the stop test (the longdouble twin of a float64 run whose count nothing guards)"""
    key = ("cg", name, np.dtype(dtype).name, None if iters is None else tuple(iters))
    if key not in _CACHE:
        c = inputs(ap, name)
        case = c["case"]
        out = []
        for k in range(len(case.fits)):
            x0 = None if c["X0"] is None else c["X0"][:, k]
            if iters is None:
                out.append(cg(c["A"], c["Y"][:, k], x0, case.shift, case.tol, case.maxit, dtype))
            else:
                out.append(cg(c["A"], c["Y"][:, k], x0, case.shift, 0.0, iters[k], dtype))
        _CACHE[key] = out
    return _CACHE[key]


def reference(ap, name):
    """the longdouble restatement of every fit at the float64 restatement's iteration count: the two may stop an
    iteration or two apart on their own (rounding delays the float64 recurrence), and x is compared at equal count"""
    return restated(ap, name, np.longdouble, iters=[r["iters"] for r in restated(ap, name, np.float64)])


STATE = ("iters", "total", "capped", "done", "brk", "zero")  # the six values per fit of admm_op_spmm_cg's state


def operator(ap, D, Y, X0=None, shift=0.0, tol=1e-10, maxit=200, batch=0, stop=None, K=None, raw=None):
    """admm_op_spmm_cg on copies of the inputs: (rc, dict(X, R n x K, state K x 6, next_batch and one int array per name
    of STATE)).  D: a scipy.sparse matrix, or a ready admm_sparse_desc with cols = Y.shape[0].  raw: arguments by name
    that replace the ones built here (a None pointer, for the refusals)"""
    import ctypes as C

    from sparse_cases import csc_of, desc_of
    L = ap._lib
    csc = None
    if hasattr(D, "tocsc"):
        csc = csc_of(D)
        D = desc_of(L, csc)
    Y = np.asfortranarray(Y, dtype=np.float64)
    n, Kc = Y.shape
    K = Kc if K is None else K
    X = np.full((n, Kc), np.nan, order="F")
    R = np.full((n, Kc), np.nan, order="F")
    state = np.full((Kc, 6), -1, dtype=np.int64)
    nb = C.c_int32(-1)
    X0c = None if X0 is None else np.asfortranarray(X0, dtype=np.float64)
    stopc = None if stop is None else np.ascontiguousarray(stop, dtype=np.int32)
    a = dict(D=C.byref(D), Y=L.as_dp(Y), X0=None if X0c is None else L.as_dp(X0c),
             stop=None if stopc is None else stopc.ctypes.data_as(C.POINTER(C.c_int32)), X=L.as_dp(X), R=L.as_dp(R),
             state=state.ctypes.data_as(C.POINTER(C.c_int64)), next_batch=C.byref(nb))
    a.update(raw or {})
    rc = L.load().admm_op_spmm_cg(a["D"], K, a["Y"], a["X0"], shift, tol, maxit, batch, a["stop"], a["X"], a["R"],
                                  a["state"], a["next_batch"])
    out = dict(X=X, R=R, state=state, next_batch=nb.value, keep=(csc, X0c, stopc))
    out.update({name: state[:, j] for j, name in enumerate(STATE)})
    return rc, out


def run_case(ap, name, **over):
    """the operator on the inputs of a case; raises on a refusal"""
    c = inputs(ap, name)
    case = c["case"]
    kw = dict(X0=c["X0"], shift=case.shift, tol=case.tol, maxit=case.maxit)
    kw.update(over)
    rc, out = operator(ap, c["D"], c["Y"], **kw)
    ap._lib.check(rc)
    return out
