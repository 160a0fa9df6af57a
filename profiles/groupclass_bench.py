"""Group penalties on the sparse linear classifiers: the ungrouped object against groups of 10 and groups
of 1000 on the same matrix in the same process -- dense 12000 x 10000 (L1Classifier) and sparse 100000 x 10000 at 1 % and
0.1 % density (SparseL1Classifier), logistic loss, ten lambda log-spaced from lambda_max to 0.01 lambda_max.

Per leg: microseconds per ADMM iteration from the loop's own event-timed runtime over a forced run length (domaxiters,
five iterations by default; the median of --reps runs with their spread); on the sparse object also the element kernel
alone (kernel_time); and ten runs of a one-fit object with groups as the other leg.  Every GPU step runs under its own
time limit: a watchdog ends the process with status 124 if a step overruns it.

    python profiles/groupclass_bench.py [--legs dense,sparse] [--dense 12000x10000] [--sparse 100000x10000]
                                        [--densities 0.01,0.001] [--iters 5] [--reps 5] [--out f.json]
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

GROUPINGS = (("ungrouped", None), ("groups of 10", 10), ("groups of 1000", 1000))


def measure(obj, iters, reps):
    go = lambda: obj.run(domaxiters=1, maxiters=iters, nodualerror=1)["runtime"]
    go()  # warm-up
    ts = [go() / iters * 1e6 for _ in range(reps)]
    return round(float(np.median(ts)), 2), round(float(min(ts)), 2), round(float(max(ts)), 2)


def legs(name, make, n, lams, args, emit, sparse):
    for label, size in GROUPINGS:
        sizes = None if size is None else [size] * (n // size) + ([n % size] if n % size else [])
        with limit(f"create, {name}, {label}", 300):
            obj = make(lams)
        try:
            if sizes is not None:
                obj.set_groups(sizes, np.sqrt(np.asarray(sizes, dtype=np.float64)))
            with limit(f"runs, {name}, {label}", 120):
                us, lo, hi = measure(obj, args.iters, args.reps)
            row = dict(leg=f"ten fits, {label}", K=10, us_per_iter=us, us_min=lo, us_max=hi)
            if sparse:
                with limit("the element kernel alone", 60):
                    row["elem_us"] = round(obj.kernel_time(20, 0)["elem_us"], 2)
            emit(**row)
        finally:
            obj.close()
    sizes = [10] * (n // 10) + ([n % 10] if n % 10 else [])
    with limit(f"create, {name}, one fit", 300):
        obj = make(lams[5:6])
    try:
        obj.set_groups(sizes, np.sqrt(np.asarray(sizes, dtype=np.float64)))
        with limit("ten runs of the one-fit object", 120):
            go = lambda: sum(obj.run(domaxiters=1, maxiters=args.iters, nodualerror=1)["runtime"] for _ in lams)
            go()
            ts = [go() / args.iters * 1e6 for _ in range(args.reps)]
        emit(leg="ten runs of the one-fit object, groups of 10", K=10, us_per_iter=round(float(np.median(ts)), 2),
             us_min=round(float(min(ts)), 2), us_max=round(float(max(ts)), 2))
    finally:
        obj.close()


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--legs", default="dense,sparse")
    a.add_argument("--dense", default="12000x10000")
    a.add_argument("--sparse", default="100000x10000")
    a.add_argument("--densities", default="0.01,0.001")
    a.add_argument("--iters", type=int, default=5)
    a.add_argument("--reps", type=int, default=5)
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    rows = []
    if "dense" in args.legs.split(","):
        m, n = (int(v) for v in args.dense.split("x"))
        p = ap.synth.sparse_classifier_problem(0, m, n)
        D, ell = p["D"], p["ell"]
        lams = ap.l1classifier_lambda_max(D, ell) * np.logspace(0.0, -2.0, 10)

        def emit(**row):
            rows.append(dict(object="dense", m=m, n=n, iters=args.iters, reps=args.reps, **row))
            print(json.dumps(rows[-1]), flush=True)

        legs("dense", lambda sel: ap.L1Classifier(D, ell, sel), n, lams, args, emit, False)
    if "sparse" in args.legs.split(","):
        m, n = (int(v) for v in args.sparse.split("x"))
        for density in (float(v) for v in args.densities.split(",")):
            p = ap.synth.sparse_design_classifier_problem(0, m, n, density)
            D, ell = p["D"], p["ell"]
            lams = ap.l1classifier_lambda_max(D, ell) * np.logspace(0.0, -2.0, 10)

            def emit(**row):
                rows.append(dict(object="sparse", m=m, n=n, density=density, nnz=int(D.nnz), iters=args.iters,
                                 reps=args.reps, **row))
                print(json.dumps(rows[-1]), flush=True)

            legs(f"sparse {density}", lambda sel: ap.SparseL1Classifier(D, ell, sel), n, lams, args, emit, True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
