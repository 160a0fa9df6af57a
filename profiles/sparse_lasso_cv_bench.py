"""Cross-validation of the lasso's path on a sparse design matrix, all legs in one process, at
100000 x 10000 with density 1 % and 0.1 %, a forced run length (domaxiters), medians of --reps runs:

  (a) lasso_cv with F = 5 folds and L = 10 lambdas: 60 fits in one object, D uploaded once (wall clock of the call, and
      the loop's own event-timed runtime);
  (b) six lasso_path runs on host-built row-subset matrices (five training sets and the full data), host slicing and
      uploads included -- what a user had to do before;
  (c) the row-weighted store's cost: the loop of one 60-fit object with observations set (every forward product of the
      CG through the weighted launch) against the same object without them, per lock-step inner iteration.

    python profiles/sparse_lasso_cv_bench.py [--shape 100000x10000] [--iters 5] [--reps 5] [--cg-maxit 30] [--out f.json]
prints one JSON line per density.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402

F, L = 5, 10


def median_spread(ts):
    return float(np.median(ts)), float(max(ts) - min(ts))


def leg(name, p, args):
    D, s = p["D"].tocsc(), p["s"]
    m = D.shape[0]
    lmax = float(np.max(np.abs(D.T @ s)))
    lams = lmax * np.logspace(0.0, -2.0, L)
    foldid = ap.solvers.cv_folds(m, F, 0)
    loop = dict(domaxiters=1, maxiters=args.iters, cg_maxit=args.cg_maxit)

    def cv():
        t0 = time.perf_counter()
        r = ap.lasso_cv(D, s, lams, dict(loop, nfolds=F, foldid=foldid))
        return time.perf_counter() - t0, r["runtime"]

    def six_paths():
        t0 = time.perf_counter()
        loops = 0.0
        csr = D.tocsr()
        for f in range(F + 1):
            rows = np.flatnonzero(foldid != f)
            Df = D if f == F else csr[rows].tocsc()
            frac = rows.size / m
            loops += ap.lasso_path(Df, s[rows], lams * frac, dict(loop))["runtime"]
        return time.perf_counter() - t0, loops

    cv()  # warm-up
    a = [cv() for _ in range(args.reps)]
    six_paths()
    b = [six_paths() for _ in range(args.reps)]

    # (c) one object of 60 fits, the same lambdas, with and without the row weights
    lam60 = np.tile(lams, F + 1)
    held = np.concatenate([np.repeat(np.arange(F), L), np.full(L, -1)])
    obj = ap.SparseLassoMulti(D, s, lam60)
    try:
        def timed():
            obj.run(**loop)
            runs = [obj.run(**loop) for _ in range(args.reps)]
            inner = int(runs[-1]["cg_iters_total"].max())
            t, spread = median_spread([r["runtime"] for r in runs])
            return t, spread, inner
        plain = timed()
        obj.set_observations(None, foldid, held)
        folds = timed()
        obj.set_observations(np.ones(m), foldid, held)
        both = timed()
    finally:
        obj.close()

    r = lambda v: round(float(v), 3)
    wall_a, sp_a = median_spread([t for t, _ in a])
    wall_b, sp_b = median_spread([t for t, _ in b])
    row = dict(leg=name, m=m, n=D.shape[1], nnz=int(D.nnz), folds=F, nlambda=L, admm_iters=args.iters,
               cg_maxit=args.cg_maxit, reps=args.reps,
               cv_wall_ms=r(wall_a * 1e3), cv_wall_spread_ms=r(sp_a * 1e3), cv_loop_ms=r(np.median([t for _, t in a]) * 1e3),
               six_paths_wall_ms=r(wall_b * 1e3), six_paths_wall_spread_ms=r(sp_b * 1e3),
               six_paths_loop_ms=r(np.median([t for _, t in b]) * 1e3), wall_speedup=r(wall_b / wall_a),
               plain_loop_ms=r(plain[0] * 1e3), plain_spread_ms=r(plain[1] * 1e3), plain_inner=plain[2],
               plain_us_per_inner=r(plain[0] / max(plain[2], 1) * 1e6),
               folds_loop_ms=r(folds[0] * 1e3), folds_spread_ms=r(folds[1] * 1e3), folds_inner=folds[2],
               folds_us_per_inner=r(folds[0] / max(folds[2], 1) * 1e6),
               weights_loop_ms=r(both[0] * 1e3), weights_spread_ms=r(both[1] * 1e3), weights_inner=both[2],
               weights_us_per_inner=r(both[0] / max(both[2], 1) * 1e6))
    print(json.dumps(row), flush=True)
    return row


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--shape", default="100000x10000")
    a.add_argument("--iters", type=int, default=5)
    a.add_argument("--reps", type=int, default=5)
    a.add_argument("--cg-maxit", type=int, default=30)
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    m, n = (int(v) for v in args.shape.split("x"))
    rows = []
    for name, density, seed in (("1 %", 0.01, 0), ("0.1 %", 0.001, 1)):
        rows.append(leg(name, ap.synth.sparse_lasso_problem(seed, m, n, density), args))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
