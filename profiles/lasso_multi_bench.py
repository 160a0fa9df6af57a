"""The lasso over several lambda values on a DENSE design matrix: one, five and ten lambda through the
multi-fit object (the cached inverse read once per chunk of fits) against ten runs of the ``lasso`` engine (one fit per
run, the packed single-vector x-solve) on the same matrix in the same process, at 12000 x 10000 (the shape of
penalty_bench.py).

Per leg: microseconds per iteration from the loop's own event-timed runtime over a forced run length (domaxiters, five
iterations by default; the median of --reps runs with their spread).  Then the product kernel alone (tile pass +
partial-row sum on the object's own buffers), event-timed, with the bytes it streams and the FMAs it issues.  Every GPU
step runs under its own time limit: a watchdog ends the process with status 124 if a step overruns it.

    python profiles/lasso_multi_bench.py [--shape 12000x10000] [--iters 5] [--reps 5] [--out f.json]
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
    a.add_argument("--shape", default="12000x10000")
    a.add_argument("--iters", type=int, default=5)
    a.add_argument("--reps", type=int, default=5)
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    L = ap._lib
    m, n = (int(v) for v in args.shape.split("x"))
    p = ap.synth.lasso_problem(0, m, n)
    D, s = p["D"], p["s"]
    lmax = float(np.max(np.abs(D.T @ s)))
    lams = lmax * np.logspace(-0.1, -2.0, 10)
    rows = []

    def emit(**row):
        rows.append(dict(m=m, n=n, iters=args.iters, reps=args.reps, **row))
        print(json.dumps(rows[-1]), flush=True)

    for name, sel in (("one fit in one object", lams[5:6]), ("five fits in one object", lams[::2]),
                      ("ten fits in one object", lams)):
        with limit(f"create, {name}", 240):
            obj = ap.LassoMulti(D, s, sel)
        try:
            with limit(f"runs, {name}", 120):
                us, lo, hi = per_iter_us(lambda: obj.run(domaxiters=1, maxiters=args.iters)["runtime"], args.iters, args.reps)
                xs = obj.xsolve
            emit(leg=name, K=int(sel.size), xsolve=xs, us_per_iter=us, us_min=lo, us_max=hi)
            if sel.size == 10 and xs == "inverse":
                with limit("the product kernel alone", 60):
                    t = obj.product_time(20)
                emit(leg="product kernel alone, ten fits", K=10, us_per_call=round(t["us"], 2),
                     stored_bytes=t["stored_bytes"], fma=t["fma"],
                     stored_TB_per_s=round(t["stored_bytes"] / t["us"] / 1e6, 2), TFMA_per_s=round(t["fma"] / t["us"] / 1e6, 2))
        finally:
            obj.close()

    with limit("create, the lasso engine", 240):
        eng = ap.Engine(L.PROB_LASSO, D=D, s=s, lam=float(lams[0]))
    try:
        eng.set_profiling(False)
        kw = dict(domaxiters=1, record_history=0, maxiters=args.iters)
        with limit("ten runs of the lasso engine", 180):
            us, lo, hi = per_iter_us(lambda: sum(eng.run(**kw).runtime_s for _ in lams), args.iters, args.reps)
            info = eng.info()
        emit(leg="ten runs of the lasso engine", K=10, xsolve=info["xsolve_used"], us_per_iter=us, us_min=lo, us_max=hi,
             us_per_iter_and_fit=round(us / 10.0, 2))
    finally:
        eng.close()
    ten = next(r for r in rows if r["leg"] == "ten fits in one object")
    emit(leg="ten fits: one object against ten engine runs",
         ratio=round(rows[-1]["us_per_iter"] / ten["us_per_iter"], 2))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
