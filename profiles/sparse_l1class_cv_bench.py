"""Cross-validation of the l1-regularised logistic regression's path on a sparse design matrix, all legs
in one process, at 100000 x 10000 with density 1 % and 0.1 %, a forced run length (domaxiters), medians of --reps runs:

  (a) l1classifier_cv with F = 5 folds and L = 10 lambdas: 60 fits in one object, D uploaded once (wall clock of the
      call, and the loop's own event-timed runtime);
  (b) six l1classifier_path runs on host-built row-subset matrices (five training sets and the full data), host slicing
      and uploads included -- what a user had to do before;
  (c) the row kernel alone, event-timed through kernel_time, on one 60-fit object without folds and with them (the FOLD
      form: 4 B more per row and a select), and the loop of that object without and with folds.

    python profiles/sparse_l1class_cv_bench.py [--shape 100000x10000] [--iters 5] [--reps 5] [--cg-maxit 30] [--out f.json]
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
    D, ell = p["D"].tocsc(), p["ell"]
    m = D.shape[0]
    lmax = ap.l1classifier_lambda_max(D, ell)
    lams = lmax * np.logspace(0.0, -2.0, L)
    foldid = ap.solvers.cv_folds(m, F, 0)
    loop = dict(domaxiters=1, maxiters=args.iters, cg_maxit=args.cg_maxit, nodualerror=1)

    def cv():
        t0 = time.perf_counter()
        r = ap.l1classifier_cv(D, ell, lams, dict(loop, nfolds=F, foldid=foldid))
        return time.perf_counter() - t0, r["runtime"]

    def six_paths():
        t0 = time.perf_counter()
        loops = 0.0
        csr = D.tocsr()
        for f in range(F + 1):
            rows = np.flatnonzero(foldid != f)
            Df = D if f == F else csr[rows].tocsc()
            loops += ap.l1classifier_path(Df, ell[rows], lams * (rows.size / m), dict(loop))["runtime"]
        return time.perf_counter() - t0, loops

    cv()  # warm-up
    a = [cv() for _ in range(args.reps)]
    six_paths()
    b = [six_paths() for _ in range(args.reps)]

    lam60 = np.tile(lams, F + 1)
    held = np.concatenate([np.repeat(np.arange(F), L), np.full(L, -1)])
    obj = ap.SparseL1Classifier(D, ell, lam60)
    try:
        def timed():
            obj.run(**loop)
            t, spread = median_spread([obj.run(**loop)["runtime"] for _ in range(args.reps)])
            return t, spread, obj.kernel_time(20, 0)["row_us"]
        plain = timed()
        obj.set_folds(foldid, held)
        folds = timed()
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
               plain_loop_ms=r(plain[0] * 1e3), plain_spread_ms=r(plain[1] * 1e3), plain_row_us=r(plain[2]),
               folds_loop_ms=r(folds[0] * 1e3), folds_spread_ms=r(folds[1] * 1e3), folds_row_us=r(folds[2]))
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
        rows.append(leg(name, ap.synth.sparse_design_classifier_problem(seed, m, n, density), args))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
