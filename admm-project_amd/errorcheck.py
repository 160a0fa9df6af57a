"""Host-side validation helpers mirroring /root/reference/errorcheck.m.

Only ``slicemaker`` (errorcheck.m:216-267) shapes the hot path: it defines the row
partition used by consensus lasso and by the transpose-reduction (row-sharded) engines.
"""
from __future__ import annotations

import numpy as np


def slicemaker(slices, workers, length):
    """Balance a slice specification over ``workers`` (errorcheck.m:216-267).

    * scalar 0  -> ``floor(len/workers)`` rows each, the first ``mod(len, workers)`` slices
      get one extra row (errorcheck.m:249-259);
    * scalar k>0 -> blocks of k rows, last block the remainder.  Deviation q13 (documented):
      the reference overwrites the last full block with ``mod(len,k) = 0`` when k divides
      len; we return the evenly divided blocks instead;
    * vector    -> must sum to ``length`` (errorcheck.m:263-265).
    """
    sl = np.atleast_1d(np.asarray(slices))
    if sl.dtype.kind not in "iuf":
        raise TypeError("Argument slices is not a numeric vector or integer!")
    sl = np.floor(np.real(sl)).astype(np.int64)
    length = int(length)
    workers = int(workers)
    if sl.size == 1 and sl[0] > 0:
        size = int(sl[0])
        out = [size] * (length // size)
        if length % size:
            out.append(length % size)
        return out
    if sl.size == 1 and sl[0] == 0:
        if workers <= 0:
            raise ValueError("There are no workers on this machine, cannot perform parallel ADMM!")
        rem = length % workers
        size = length // workers
        return [size + 1] * rem + [size] * (workers - rem)
    if int(sl.sum()) != length:
        raise ValueError("The number of parallel slices does not match length of x!")
    return [int(k) for k in sl]


def slice_ranges(slices):
    """0-based [lo, hi) row ranges of consecutive slices (getProxOps.m:402-412)."""
    starts = np.concatenate([[0], np.cumsum(np.asarray(slices, dtype=np.int64))])
    return [(int(starts[i]), int(starts[i + 1])) for i in range(len(slices))]


def rank_rows(length, rank, nranks):
    """Row range of ``rank`` when ``length`` rows are sharded over ``nranks`` devices with
    slicemaker(0, nranks, length)."""
    return slice_ranges(slicemaker(0, nranks, length))[rank]


def is_nonnegative_real(v, name):
    if not np.isscalar(v) or not np.isreal(v) or v < 0:
        raise ValueError(f"Argument {name} is not a nonnegative real number!")
    return float(v)


def is_positive_real(v, name):
    if not np.isscalar(v) or not np.isreal(v) or v <= 0:
        raise ValueError(f"Argument {name} is not a positive real number!")
    return float(v)


def group_sizes(groups, weights, n):
    """args.groups / args.groupweights of group lasso: sizes as int64 (each an integer >= 1, summing to n) and the
    weights as float64 (one finite value >= 0 per group) or None.  Raises before any device work."""
    g = np.asarray(groups, dtype=np.float64).reshape(-1)
    if g.size == 0:
        raise ValueError("groups must hold at least one group size")
    if not np.all(np.isfinite(g)) or np.any(g != np.floor(g)):
        raise ValueError("groups: every size must be an integer")
    if np.any(g < 1):
        raise ValueError("groups: every size must be >= 1")
    if int(g.sum()) != int(n):
        raise ValueError(f"groups: the sizes sum to {int(g.sum())}, not to the {int(n)} columns of D")
    w = None
    if weights is not None:
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        if w.size != g.size:
            raise ValueError(f"groupweights has {w.size} entries for {g.size} groups")
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError("groupweights: every weight must be finite and >= 0")
    return np.ascontiguousarray(g.astype(np.int64)), w


LOSS_KEYS = ("weights", "tau", "slopes", "epsilon", "delta")


def loss_fields(src, m, kind):
    """The loss family of lad / huberfit (admm_engine_set_loss) out of a dict of args / options: ``weights`` (m finite
    values >= 0), ``tau`` (strictly inside (0, 1): slopes (tau, 1 - tau)) or ``slopes`` (two finite values > 0),
    ``epsilon`` (finite, >= 0; lad only) and ``delta`` (finite, > 0; huberfit only).  Returns Engine.set_loss's keyword
    arguments for the fields that were given (None where none was).  Raises before any device work."""
    given = {k: src[k] for k in LOSS_KEYS if src.get(k) is not None}
    if not given:
        return None
    out = {}
    if "weights" in given:
        w = np.ascontiguousarray(np.asarray(given["weights"], dtype=np.float64).reshape(-1))
        if w.size != int(m):
            raise ValueError(f"weights has {w.size} entries for the {int(m)} rows of D")
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError("weights: every weight must be finite and >= 0")
        out["weights"] = w
    if "tau" in given and "slopes" in given:
        raise ValueError("tau beside slopes: give one of them")
    if "tau" in given:
        tau = given["tau"]
        if not np.isscalar(tau) or not np.isreal(tau) or not 0.0 < tau < 1.0:
            raise ValueError("tau must lie strictly inside (0, 1)")
        out["slopes"] = (float(tau), 1.0 - float(tau))
    if "slopes" in given:
        sl = np.asarray(given["slopes"], dtype=np.float64).reshape(-1)
        if sl.size != 2 or not np.all(np.isfinite(sl)) or np.any(sl <= 0):
            raise ValueError("slopes must hold two finite values > 0")
        out["slopes"] = (float(sl[0]), float(sl[1]))
    for key, low_ok, owner in (("epsilon", True, "lad"), ("delta", False, "huberfit")):
        if key in given:
            v = given[key]
            if not np.isscalar(v) or not np.isreal(v) or not np.isfinite(v) or v < 0 or (v == 0 and not low_ok):
                raise ValueError(f"{key} must be a finite real number {'>= 0' if low_ok else '> 0'}")
            if kind != owner and v != (0.0 if low_ok else 1.0):
                raise ValueError(f"{key} belongs to {owner}, not to {kind}")
            out[key] = float(v)
    return out


SVM_COST_KEYS = ("weights", "classcost")


def svm_cost_fields(src, ell):
    """The costs of linearsvm (admm_engine_set_svm_cost) out of a dict of args / options: ``weights`` (m finite values
    >= 0) and ``classcost``, a pair (pos, neg) of finite values >= 0 or 'balanced' -> (m/(2*m_pos), m/(2*m_neg)) from the
    signs of ``ell``.  Returns Engine.set_svm_cost's keyword arguments for the fields that were given (None where none
    was).  Raises before any device work."""
    given = {k: src[k] for k in SVM_COST_KEYS if src.get(k) is not None}
    if not given:
        return None
    ell = np.asarray(ell, dtype=np.float64).reshape(-1)
    out = {}
    if "weights" in given:
        w = np.ascontiguousarray(np.asarray(given["weights"], dtype=np.float64).reshape(-1))
        if w.size != ell.size:
            raise ValueError(f"weights has {w.size} entries for the {ell.size} rows of D")
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError("weights: every weight must be finite and >= 0")
        out["weights"] = w
    if "classcost" in given:
        out["classcost"] = class_cost_pair(given["classcost"], ell)
    return out


def class_cost_pair(cc, ell):
    """(pos, neg) out of options.classcost: a pair of finite values >= 0, or 'balanced' from the label counts of ell"""
    if isinstance(cc, str):
        if cc.lower() != "balanced":
            raise ValueError("classcost is neither a pair (pos, neg) nor 'balanced'")
        m, mp = ell.size, int(np.sum(ell > 0))
        if mp == 0 or mp == m:
            raise ValueError("classcost = 'balanced' needs observations of both classes")
        return (m / (2.0 * mp), m / (2.0 * (m - mp)))
    try:
        pair = np.asarray(cc, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("classcost is neither a pair (pos, neg) nor 'balanced'") from None
    if pair.size != 2 or not np.all(np.isfinite(pair)) or np.any(pair < 0):
        raise ValueError("classcost must hold two finite values >= 0 (positive class, negative class)")
    return (float(pair[0]), float(pair[1]))


PENALTY_KEYS = ("l1weights", "ridge", "nonnegative", "l1")


def penalty_fields(src, n):
    """The penalty family of a lasso (admm_engine_set_penalty) out of a dict of args / options: ``l1weights`` (n finite
    values >= 0), ``ridge`` and ``l1`` (finite, >= 0), ``nonnegative`` (0 or 1).  Returns the checked fields that were
    given (None where none was).  Raises before any device work."""
    given = {k: src[k] for k in PENALTY_KEYS if src.get(k) is not None}
    if not given:
        return None
    out = {}
    if "l1weights" in given:
        w = np.ascontiguousarray(np.asarray(given["l1weights"], dtype=np.float64).reshape(-1))
        if w.size != int(n):
            raise ValueError(f"l1weights has {w.size} entries for the {int(n)} columns of D")
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError("l1weights: every weight must be finite and >= 0")
        out["l1weights"] = w
    for key in ("ridge", "l1"):
        if key in given:
            v = given[key]
            if not np.isscalar(v) or not np.isreal(v) or not np.isfinite(v) or v < 0:
                raise ValueError(f"{key} must be a finite real number >= 0")
            out[key] = float(v)
    if "nonnegative" in given:
        v = given["nonnegative"]
        if isinstance(v, (bool, np.bool_)):
            v = int(v)
        if not np.isscalar(v) or v not in (0, 1):
            raise ValueError("nonnegative must be 0 or 1")
        out["nonnegative"] = int(v)
    return out
