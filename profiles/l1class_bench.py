"""Sparse linear classifiers over several lambda values on a DENSE design matrix: ten, five and one
lambda in one object (D read twice per iteration and chunk of fits) against ten runs of the one-fit object on the same
matrix in the same process, at 12000 x 10000 and 60000 x 400, logistic loss.

Per leg: microseconds per iteration from the loop's own event-timed runtime over a forced run length (domaxiters, five
iterations by default; the median of --reps runs with their spread).  Then the two passes over D alone (one chunk, the
element update included; the transposed pass with one and with three vectors per fit), event-timed, against the bytes of
D: the rate to hold against a pure read of D (csrc/dev/read_bw.hip).  Every GPU step runs under its own time limit: a
watchdog ends the process with status 124 if a step overruns it.

    python profiles/l1class_bench.py [--shapes 12000x10000,60000x400] [--iters 5] [--reps 5] [--out f.json]
prints one JSON line per leg.
"""
import argparse
import json
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402


class limit:
    """a GPU step with a time limit of its own: the process ends (status 124) when the step overruns it"""

    def __init__(self, what, seconds):
        self.what, self.seconds = what, seconds

    def __enter__(self):
        def overrun():
            sys.stderr.write(f"time limit: {self.what} ran longer than {self.seconds} s\n")
            sys.stderr.flush()
            os._exit(124)
        self.timer = threading.Timer(self.seconds, overrun)
        self.timer.daemon = True
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()
        return False


def per_iter_us(run, iters, reps):
    run()  # warm-up
    ts = [run() / iters * 1e6 for _ in range(reps)]
    return round(float(np.median(ts)), 2), round(float(min(ts)), 2), round(float(max(ts)), 2)


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--shapes", default="12000x10000,60000x400")
    a.add_argument("--iters", type=int, default=5)
    a.add_argument("--reps", type=int, default=5)
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    rows = []
    for shape in args.shapes.split(","):
        m, n = (int(v) for v in shape.split("x"))
        p = ap.synth.sparse_classifier_problem(0, m, n)
        D, ell = p["D"], p["ell"]
        lams = ap.l1classifier_lambda_max(D, ell) * np.logspace(-0.1, -2.0, 10)

        def emit(**row):
            rows.append(dict(m=m, n=n, iters=args.iters, reps=args.reps, **row))
            print(json.dumps(rows[-1]), flush=True)

        def run_of(obj):
            return lambda: obj.run(domaxiters=1, maxiters=args.iters)["runtime"]

        for name, sel in (("ten fits in one object", lams), ("five fits in one object", lams[::2]),
                          ("one fit in one object", lams[5:6])):
            with limit(f"create, {name}", 300):
                obj = ap.L1Classifier(D, ell, sel)
            try:
                with limit(f"runs, {name}", 120):
                    us, lo, hi = per_iter_us(run_of(obj), args.iters, args.reps)
                emit(leg=name, K=int(sel.size), xsolve=obj.xsolve, us_per_iter=us, us_min=lo, us_max=hi)
                if sel.size == 10:
                    ten = us
                    for nvec in (1, 3):
                        with limit("the passes alone", 60):
                            t = obj.pass_time(20, nvec)
                        emit(leg=f"the passes alone, ten fits, {nvec} vector(s) per fit in the transposed pass", K=10,
                             forward_us=round(t["forward_us"], 2), transposed_us=round(t["transposed_us"], 2),
                             d_bytes=t["d_bytes"], forward_TB_per_s=round(t["d_bytes"] / t["forward_us"] / 1e6, 2),
                             transposed_TB_per_s=round(t["d_bytes"] / t["transposed_us"] / 1e6, 2))
                if sel.size == 1:
                    with limit("ten runs of the one-fit object", 120):
                        us, lo, hi = per_iter_us(lambda: sum(run_of(obj)() for _ in lams), args.iters, args.reps)
                    emit(leg="ten runs of the one-fit object", K=10, us_per_iter=us, us_min=lo, us_max=hi,
                         us_per_iter_and_fit=round(us / 10.0, 2))
                    emit(leg="ten fits: one object against ten one-fit runs", ratio=round(us / ten, 2))
            finally:
                obj.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
