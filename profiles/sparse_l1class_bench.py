"""Sparse linear classifiers over several lambda values on a SPARSE design matrix: ten, five and one
lambda in one object (one sparse product serves ten fits) against ten runs of the one-fit object on the same matrix in
the same process, at 100000 x 10000 with 1 % and 0.1 % density, logistic loss, lambda log-spaced from lambda_max to
0.01 lambda_max.

Per leg: microseconds per ADMM iteration from the loop's own event-timed runtime over a forced run length (domaxiters,
five iterations by default; the median of --reps runs with their spread), the lock-step inner iterations per ADMM
iteration and microseconds per inner iteration -- with nodualerror = 1 and, for the ten-fit object, with nodualerror = 0
(two more transposed products per iteration).  Then the row kernel and the element kernel alone, event-timed.  Every GPU
step runs under its own time limit: a watchdog ends the process with status 124 if a step overruns it.

    python profiles/sparse_l1class_bench.py [--shape 100000x10000] [--densities 0.01,0.001] [--iters 5] [--reps 5] [--out f.json]
prints one JSON line per leg.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402
from l1class_bench import limit  # noqa: E402


def measure(obj, iters, reps, nodualerror):
    """(median, min, max) microseconds per ADMM iteration, and the lock-step inner iterations of one run"""
    go = lambda: obj.run(domaxiters=1, maxiters=iters, nodualerror=nodualerror)
    go()  # warm-up
    runs = [go() for _ in range(reps)]
    ts = [r["runtime"] / iters * 1e6 for r in runs]
    inner = int(runs[0]["cg_iters_total"].max())  # (the longest fit sets the number of lock-step iterations)
    return round(float(np.median(ts)), 2), round(float(min(ts)), 2), round(float(max(ts)), 2), inner


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--shape", default="100000x10000")
    a.add_argument("--densities", default="0.01,0.001")
    a.add_argument("--iters", type=int, default=5)
    a.add_argument("--reps", type=int, default=5)
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    m, n = (int(v) for v in args.shape.split("x"))
    rows = []
    for density in (float(v) for v in args.densities.split(",")):
        p = ap.synth.sparse_design_classifier_problem(0, m, n, density)
        D, ell = p["D"], p["ell"]
        lams = ap.l1classifier_lambda_max(D, ell) * np.logspace(0.0, -2.0, 10)

        def emit(**row):
            rows.append(dict(m=m, n=n, density=density, nnz=int(D.nnz), iters=args.iters, reps=args.reps, **row))
            print(json.dumps(rows[-1]), flush=True)

        for name, sel in (("ten fits in one object", lams), ("five fits in one object", lams[::2]),
                          ("one fit in one object", lams[5:6])):
            with limit(f"create, {name}", 120):
                obj = ap.SparseL1Classifier(D, ell, sel)
            try:
                for nd in ((1, 0) if sel.size == 10 else (1,)):
                    with limit(f"runs, {name}", 120):
                        us, lo, hi, inner = measure(obj, args.iters, args.reps, nd)
                    emit(leg=name, K=int(sel.size), nodualerror=nd, us_per_iter=us, us_min=lo, us_max=hi,
                         inner_per_iter=round(inner / args.iters, 2), us_per_inner=round(us * args.iters / max(inner, 1), 2))
                    if sel.size == 10 and nd == 1:
                        ten = us
                if sel.size == 10:
                    with limit("the element kernels alone", 60):
                        t = obj.kernel_time(20, 1)
                    emit(leg="the row kernel and the element kernel alone, ten fits", K=10, row_us=round(t["row_us"], 2),
                         elem_us=round(t["elem_us"], 2))
                if sel.size == 1:
                    with limit("ten runs of the one-fit object", 120):
                        go = lambda: sum(obj.run(domaxiters=1, maxiters=args.iters, nodualerror=1)["runtime"] for _ in lams)
                        go()
                        ts = [go() / args.iters * 1e6 for _ in range(args.reps)]
                    us = round(float(np.median(ts)), 2)
                    emit(leg="ten runs of the one-fit object", K=10, nodualerror=1, us_per_iter=us,
                         us_min=round(min(ts), 2), us_max=round(max(ts), 2))
                    emit(leg="ten fits: ten one-fit runs against one object", ratio=round(us / ten, 2))
            finally:
                obj.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
