"""The multinomial (softmax) model on a SPARSE design matrix against the same object with
set_multinomial(0) -- ten one-vs-rest logistic fits over the same products -- at 100000 x 10000 with 1 % and 0.1 %
density, Cn = 10 classes, in one process.

Per leg: microseconds per ADMM iteration from the loop's own event-timed runtime over a forced run length (domaxiters,
five iterations by default; the median of --reps runs with their spread) and the lock-step inner iterations per ADMM
iteration, with nodualerror = 1 and 0.  Then the row kernel the object would run and the element kernel alone,
event-timed, in both forms.  Every GPU step runs under its own time limit: a watchdog ends the process with status 124
if a step overruns it.

    python profiles/sparse_multinomial_bench.py [--shape 100000x10000] [--densities 0.01,0.001] [--classes 10] [--iters 5] [--reps 5] [--out f.json]
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
from sparse_l1class_bench import measure  # noqa: E402


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--shape", default="100000x10000")
    a.add_argument("--densities", default="0.01,0.001")
    a.add_argument("--classes", type=int, default=10)
    a.add_argument("--iters", type=int, default=5)
    a.add_argument("--reps", type=int, default=5)
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    m, n = (int(v) for v in args.shape.split("x"))
    Cn = args.classes
    rows = []
    for density in (float(v) for v in args.densities.split(",")):
        p = ap.synth.sparse_multinomial_problem(0, m, n, density, Cn)
        D, y = p["D"], p["y"]
        lam = 0.1 * ap.multinomial_lambda_max(D, y)
        first, K = ap.softmax.slot_map(1, Cn)
        ELL = np.asfortranarray(np.where(y[:, None] == np.arange(Cn)[None, :], 1.0, -1.0))

        def emit(**row):
            rows.append(dict(m=m, n=n, density=density, nnz=int(D.nnz), classes=Cn, iters=args.iters, reps=args.reps, **row))
            print(json.dumps(rows[-1]), flush=True)

        with limit("create", 120):
            obj = ap.SparseL1Classifier(D, ELL, np.full(K, lam))
        try:
            us = {}
            for name, classes in (("multinomial model", Cn), ("ten one-vs-rest logistic fits", 0)):
                obj.set_multinomial(classes)
                for nd in (1, 0):
                    with limit(f"runs, {name}", 120):
                        t, lo, hi, inner = measure(obj, args.iters, args.reps, nd)
                    us[(classes, nd)] = t
                    emit(leg=name, nodualerror=nd, us_per_iter=t, us_min=lo, us_max=hi,
                         inner_per_iter=round(inner / args.iters, 2))
                with limit("the element kernels alone", 60):
                    k = obj.kernel_time(20, 1)
                emit(leg=f"the row kernel and the element kernel alone, {name}", row_us=round(k["row_us"], 2),
                     elem_us=round(k["elem_us"], 2))
            for nd in (1, 0):
                emit(leg="multinomial against one-vs-rest, per iteration", nodualerror=nd,
                     ratio=round(us[(Cn, nd)] / us[(0, nd)], 3))
        finally:
            obj.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
