"""Quantile regression on a sparse design matrix: K = 5 and 10 quantiles in one object against K runs of
the K = 1 object in the same process, at 100000 x 10000 with density 1 % and 0.1 %, and the K = 10 object with the dual
residual on (nodualerror = 0: two more transposed products per iteration) against off.

Per leg: the loop's own event-timed runtime (a forced run length) as the median of --reps runs with their spread,
microseconds per ADMM iteration and per lock-step inner iteration (runtime / the largest per-fit inner count).

    python profiles/sparse_reg_bench.py [--shape 100000x10000] [--iters 5] [--reps 3] [--cg-maxit 30] [--out file.json]
prints one JSON line per leg.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402


def timed(obj, args, z0, u0, nodualerror=1):
    kw = dict(domaxiters=1, maxiters=args.iters, cg_maxit=args.cg_maxit, nodualerror=nodualerror, z0=z0, u0=u0)
    obj.run(**kw)  # warm-up
    runs = [obj.run(**kw) for _ in range(args.reps)]
    ts = [r["runtime"] for r in runs]
    return float(np.median(ts)), float(max(ts) - min(ts)), runs[-1]


def make(D, s, taus):
    taus = np.asarray(taus, dtype=np.float64)
    return ap.SparseRegMulti(D, s, [0] * taus.size, taus, 1.0 - taus)


def leg(name, p, K, args):
    D, s, m, n = p["D"], p["s"], p["D"].shape[0], p["D"].shape[1]
    taus = np.linspace(0.05, 0.95, K)
    rng = np.random.default_rng(3)
    z0, u0 = np.asfortranarray(rng.random((m, K))), np.asfortranarray(rng.random((m, K)))
    obj = make(D, s, taus)
    try:
        t, spread, last = timed(obj, args, z0, u0)
        td, spread_d, _ = timed(obj, args, z0, u0, nodualerror=0)
    finally:
        obj.close()
    t1 = 0.0  # the same K quantiles as K runs of the one-fit object
    for c in range(K):
        one = make(D, s, taus[c:c + 1])
        try:
            t1 += timed(one, args, z0[:, c:c + 1], u0[:, c:c + 1])[0]
        finally:
            one.close()
    inner = int(last["cg_iters_total"].max())
    row = dict(leg=name, m=m, n=n, nnz=int(D.nnz), K=K, chunk=ap.SparseRegMulti.chunk(), admm_iters=args.iters,
               inner_iters=inner, ms_K_fits=round(t * 1e3, 2), spread_ms=round(spread * 1e3, 2),
               ms_K_single_runs=round(t1 * 1e3, 2), speedup=round(t1 / t, 2),
               ms_K_fits_dual=round(td * 1e3, 2), spread_dual_ms=round(spread_d * 1e3, 2),
               dual_cost_percent=round((td / t - 1.0) * 100, 1),
               us_per_admm_iter=round(t / args.iters * 1e6, 1), us_per_inner_iter=round(t / max(inner, 1) * 1e6, 1),
               capped_updates=[int(v) for v in last["cg_capped_updates"]], reps=args.reps)
    print(json.dumps(row), flush=True)
    return row


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--shape", default="100000x10000")
    a.add_argument("--iters", type=int, default=5)
    a.add_argument("--reps", type=int, default=3)
    a.add_argument("--cg-maxit", type=int, default=30)
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    m, n = (int(v) for v in args.shape.split("x"))
    rows = []
    for name, density, seed in (("1 %", 0.01, 0), ("0.1 %", 0.001, 1)):
        p = ap.synth.sparse_lasso_problem(seed, m, n, density)  # (no intercept column: the skewed-row cost is not this leg's)
        for K in (5, 10):
            rows.append(leg(f"{name} K={K}", p, K, args))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
