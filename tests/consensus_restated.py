"""One consensus-lasso iteration tail (getProxOps.m:1281-1343) restated plainly, as the exact side of the operator
tests of consensus.hip.  Nothing here mirrors a kernel: no tiles, no slots, no summation order.

    x_k[i]   = sum_p rows[k][p][i]                       math.fsum, or int64 arithmetic for integer rows
    sx, su   = sum_k x_k, sum_k u_k  (+ the remote share)
    xave     = sx / N,  uave = su / N                    N = slices over all ranks
    z        = sign(v) * max(|v| - lambda/(rho*N), 0),   v = uave + xave
    u_k     += x_k - z
    y_k      = rho*(z - u_k) + D_k's_k
    ubar     = (uave + xave) - z                         the mean of the updated u_k
    S_R2     = sum_k ||x_k - xave||^2      S_AX2 = ||xave||^2      S_G2 = ||xave - xaveprev||^2
    S_U2     = ||ubar||^2                  S_DU2 = ||ubar - ubar_in||^2
    q        = sum_k ||x_k - c||^2         about a centre c (the sharded run: the xave that came in)

Vectors are numpy.longdouble; every scalar sum is math.fsum over longdouble terms split into two doubles, so the only
error of a sum is the 2^-64 of its terms."""
import math

import numpy as np

LD = np.longdouble
SLOT_NAMES = ("S_R2", "S_AX2", "S_G2", "S_U2", "S_DU2")


def partial_row_count(n):
    return -(-n // 128) + 1


def _fsum_ld(terms):
    """the sum of longdouble terms as a longdouble: fsum over (high, low) double halves, plus the rounding fsum left"""
    t = np.asarray(terms, dtype=LD).ravel()
    hi = t.astype(np.float64)
    lo = (t - hi.astype(LD)).astype(np.float64)
    parts = hi.tolist() + lo.tolist()
    s = math.fsum(parts)
    return LD(s) + LD(math.fsum(parts + [-s]))


def assemble(rows):
    """x_k[i] = sum_p rows[k][p][i] for rows [K][P][n].  Integer rows: int64 arithmetic, exact.  Real rows: math.fsum per
    element.  Returns (x as float64, correctly rounded; x as longdouble, float64 value + the remainder fsum reports)."""
    rows = np.asarray(rows)
    if np.issubdtype(rows.dtype, np.integer):
        x = rows.astype(np.int64).sum(axis=1)
        assert np.max(np.abs(rows).astype(np.int64).sum(axis=1)) < 2 ** 53
        return x.astype(np.float64), x.astype(LD)
    K, P, n = rows.shape
    x = np.empty((K, n))
    rem = np.empty((K, n))
    for k in range(K):
        cols = rows[k].T.tolist()
        for i, col in enumerate(cols):
            s = math.fsum(col)
            x[k, i] = s
            rem[k, i] = math.fsum(col + [-s])
    return x, x.astype(LD) + rem.astype(LD)


def slot_sums(X, xave, xaveprev, ubar, ubar_in, center=None):
    """the five sums and q (None without a centre) of the vectors given, each a longdouble"""
    X, xave, xaveprev = np.asarray(X, dtype=LD), np.asarray(xave, dtype=LD), np.asarray(xaveprev, dtype=LD)
    ubar, ubar_in = np.asarray(ubar, dtype=LD), np.asarray(ubar_in, dtype=LD)
    out = dict(S_R2=_fsum_ld((X - xave[None, :]) ** 2), S_AX2=_fsum_ld(xave ** 2),
               S_G2=_fsum_ld((xave - xaveprev) ** 2), S_U2=_fsum_ld(ubar ** 2), S_DU2=_fsum_ld((ubar - ubar_in) ** 2))
    out["q"] = None if center is None else _fsum_ld((X - np.asarray(center, dtype=LD)[None, :]) ** 2)
    return out


def consensus_tail(X, U, Dts, xave, ubar, rho, lam, Ntot, remote=None, center=None, sums=True):
    """One tail from the slices' x_k (float64 or longdouble, [K][n]).  Returns a dict of longdouble arrays X, sums
    ([2][n]), z, U, Y, xave, xaveprev, ubar, and (sums=True) the five sums under their slot names and q."""
    X, U, Dts = np.asarray(X, dtype=LD), np.asarray(U, dtype=LD), np.asarray(Dts, dtype=LD)
    xin, ubin = np.asarray(xave, dtype=LD), np.asarray(ubar, dtype=LD)
    K, n = X.shape
    assert U.shape == Dts.shape == (K, n) and xin.shape == ubin.shape == (n,) and Ntot >= K
    sx, su = X.sum(axis=0), U.sum(axis=0)
    if remote is not None:
        r = np.asarray(remote, dtype=LD)
        sx, su = sx + r[0], su + r[1]
    N = LD(Ntot)
    xnew, uave = sx / N, su / N
    v = uave + xnew
    t = LD(lam) / (LD(rho) * N)
    z = np.sign(v) * np.maximum(np.abs(v) - t, LD(0))
    Unew = U + (X - z[None, :])
    Y = LD(rho) * (z[None, :] - Unew) + Dts
    ub = v - z
    out = dict(X=X, sums=np.stack([sx, su]), z=z, U=Unew, Y=Y, xave=xnew, xaveprev=xin, ubar=ub, v=v, t=t)
    if sums:
        out.update(slot_sums(X, xnew, xin, ub, ubin, center))
    return out


def kernel_order_float64(X, U, Dts, xave, ubar, rho, lam, Ntot, remote=None):
    """The same tail in float64 NumPy in the order consensus.hip evaluates it (slice-order sums, one rounding per
    operation, no fused multiply-add): the CPU stand-in that shows the tests' rounding bound leaves fp64 room."""
    X, U, Dts = np.asarray(X, dtype=np.float64), np.asarray(U, dtype=np.float64), np.asarray(Dts, dtype=np.float64)
    K, n = X.shape
    sx, su = np.zeros(n), np.zeros(n)
    for k in range(K):
        su = su + U[k]
        sx = sx + X[k]
    if remote is not None:
        sx, su = sx + np.asarray(remote[0], dtype=np.float64), su + np.asarray(remote[1], dtype=np.float64)
    Nd = float(Ntot)
    t = lam / (rho * Nd)
    xnew, uave = sx / Nd, su / Nd
    v = uave + xnew
    p = np.maximum(np.abs(v) - t, 0.0)
    z = np.where(v > 0, p, np.where(v < 0, -p, 0.0 * p))
    Unew = U + (X - z[None, :])
    Y = rho * (z[None, :] - Unew) + Dts
    return dict(sums=np.stack([sx, su]), z=z, U=Unew, Y=Y, xave=xnew, ubar=v - z)


# ------------------------------------------------------------------------------------------------ the operator call
def call_tail(L, dp, form, n, K, Ntot, rho, lam, rows, X, U, Dts, xave, ubar, remote=None, with_q=0):
    """admm_op_consensus_tail on copies of the inputs; returns (rc, dict of float64 outputs).  Buffers the operator must
    not touch (sums with form 2, q without with_q) come back as the sentinel they were filled with."""
    sentinel = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).copy()
    rows_, U_, Dts_, xave_, ubar_, remote_ = f(rows), f(U), f(Dts), f(xave), f(ubar), f(remote)
    X_ = f(X) if form == 0 else np.full((K, n), sentinel)
    out = dict(X=X_, U=U_, xave=xave_, ubar=ubar_, Y=np.full((K, n), sentinel), sums=np.full((2, n), sentinel),
               z=np.full(n, sentinel), xaveprev=np.full(n, sentinel), slots=np.full(5, sentinel), q=np.full(1, sentinel))
    p = lambda a: None if a is None else dp(a)
    rc = L.admm_op_consensus_tail(form, n, K, Ntot, rho, lam, p(rows_), p(X_), p(U_), p(Dts_), p(xave_), p(ubar_),
                                  p(remote_), with_q, p(out["Y"]), p(out["sums"]), p(out["z"]), p(out["xaveprev"]),
                                  p(out["slots"]), p(out["q"]))
    return rc, out


def is_sentinel(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint64) == np.uint64(0x7FF8DEADBEEF0001)))


# ------------------------------------------------------------------------------------------------ the cases
IMAX = 2 ** 20
U53 = 2.0 ** -53

F2_K_SWEEP = [(2, K, 1537) for K in (1, 2, 3, 5, 7, 8, 9, 15, 16)]
F2_N_SWEEP = [(2, K, n) for K in (3, 16) for n in (1, 63, 64, 65, 127, 128, 129, 1536, 1599, 1601, 1664)]
F2_ROUND2 = [(2, 9, 2433), (2, 16, 2561), (2, 8, 5121), (2, 5, 7553)]
F2_BENCH = (2, 8, 10000)  # integer rows only
F1_SHAPES = [(1, K, 1537) for K in (1, 3, 16, 17, 33)] + [(1, 3, 129), (1, 3, 512), (1, 2, 10113)]
F0_SHAPES = [(0, K, n) for K in (1, 4, 17) for n in (1, 255, 256, 257, 70001)]


def make_case(form, K, n, kind, Ntot=None, seed=0):
    """Inputs of one tail.  kind 'int': integers in +-2^20, rho = 2, lambda = 2^22, and (n >= 8) three elements placed ON
    the kink of the threshold: v = +t, v = -t and v = 0 exactly.  kind 'real': standard normal; partial rows 0 and 1 of
    every slice cancel to 1e-8.  Form 0 draws x_k itself (rows None).  Ntot > K: a remote share, the sum of Ntot - K
    further slices drawn the same way (remote_slices keeps them for the operand scale)."""
    Ntot = K if Ntot is None else Ntot
    rng = np.random.default_rng([form, K, n, Ntot, seed, 1 if kind == "int" else 0])
    P = partial_row_count(n)
    R = Ntot - K
    if kind == "int":
        draw = lambda *s: rng.integers(-IMAX, IMAX + 1, s)
        rho, lam = 2.0, float(2 ** 22)
    else:
        draw = lambda *s: rng.standard_normal(s)
        rho = 0.7
    rows = None
    if form == 0:
        X = draw(K, n)
    else:
        rows = draw(K, P, n)
        if kind == "real":
            rows[:, 1] = -rows[:, 0] + 1e-8 * rng.standard_normal((K, n))
        X = None
    U, Dts, xave, ubar = draw(K, n), draw(K, n), draw(n), draw(n)
    rx, ru = draw(R, n), draw(R, n)  # the remote slices' x_k and u_k
    if kind == "real":
        lam = rho * Ntot * 0.67 * math.sqrt((1.0 if form == 0 else P - 1.0) / Ntot + 1.0 / Ntot)
    kinks = {}
    if kind == "int" and n >= 8:
        xs = X if form == 0 else rows.sum(axis=1)
        sx, su = xs.sum(axis=0) + rx.sum(axis=0), U.sum(axis=0) + ru.sum(axis=0)
        kinks = {1: 2 ** 21, n - 1: -(2 ** 21), n // 2: 0}  # element -> the sum of u_k that puts v there (sum x_k = 0)
        for i, target in kinks.items():
            if form == 0:
                X[0, i] -= sx[i]
            else:
                rows[0, 0, i] -= sx[i]
            U[0, i] += target - su[i]
    remote = np.stack([rx.sum(axis=0), ru.sum(axis=0)]) if R else None
    return dict(form=form, K=K, n=n, Ntot=Ntot, kind=kind, P=P, rho=rho, lam=lam, rows=rows, X=X, U=U, Dts=Dts,
                xave=xave, ubar=ubar, remote=remote, remote_slices=(rx, ru), kinks=kinks)


def operand_scale(case, X, z):
    """per element i: max over the slices of every rank of |x_k[i]|, |u_k[i]|, |D_k's_k[i]|, and |z[i]|"""
    rx, ru = case["remote_slices"]
    parts = [np.abs(np.asarray(X, dtype=LD)), np.abs(case["U"]).astype(LD), np.abs(case["Dts"]).astype(LD),
             np.abs(rx).astype(LD), np.abs(ru).astype(LD), np.abs(np.asarray(z, dtype=LD))[None, :]]
    return np.max(np.concatenate([p for p in parts if p.size], axis=0), axis=0)


def vector_ratios(case, got, ref, X):
    """max |got - ref| / bound for z, U, Y, xave, ubar: bound = 16 * 2^-53 * operand scale (* max(1, rho) for Y)"""
    scale = operand_scale(case, X, ref["z"])
    bound = 16 * LD(U53) * scale
    out = {}
    for name in ("z", "U", "Y", "xave", "ubar"):
        b = bound * max(1.0, case["rho"]) if name == "Y" else bound
        b = np.broadcast_to(b, ref[name].shape)
        err = np.abs(np.asarray(got[name], dtype=LD) - ref[name])
        if np.any(np.isnan(err)):
            out[name] = np.inf
            continue
        ok0 = (b == 0) & (err == 0)
        out[name] = float(np.max(np.where(ok0, LD(0), err / np.where(b > 0, b, LD(1)) + np.where(b > 0, LD(0), LD(np.inf)))))
    return out
