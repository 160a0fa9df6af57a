"""Group lasso over ten lambda values in one object: per-iteration time of ten GROUPED fits against ten
ungrouped fits in the same object -- the cost of the grouped element kernel over the ungrouped one -- and against ten runs
of the single-fit ``grouplasso`` engine on the same data, which is what ten group-lasso fits cost without the shared
object.  Dense 12000 x 10000 (lasso_multi_bench.py's shape) and sparse 100000 x 10000 at 1 % density
(sparse_lasso_multi_bench.py's), groups of 10 and of 1000, all legs in one process.

Per leg: microseconds per iteration from the loop's own event-timed runtime over a forced run length (domaxiters; the
median of --reps runs with their spread).  Every GPU step runs under its own time limit: a watchdog ends the process with
status 124 if a step overruns it.

    python profiles/grouplasso_multi_bench.py [--kind dense|sparse|both] [--iters 5] [--reps 5] [--out f.json]
prints one JSON line per leg.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402
from lasso_multi_bench import limit, per_iter_us  # noqa: E402

SHAPES = dict(dense=(12000, 10000, None), sparse=(100000, 10000, 0.01))
GROUPS = (10, 1000)


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--kind", default="both", choices=("dense", "sparse", "both"))
    a.add_argument("--iters", type=int, default=5)
    a.add_argument("--reps", type=int, default=5)
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    L = ap._lib
    rows = []

    def emit(**row):
        rows.append(dict(iters=args.iters, reps=args.reps, **row))
        print(json.dumps(rows[-1]), flush=True)

    for kind in (("dense", "sparse") if args.kind == "both" else (args.kind,)):
        m, n, density = SHAPES[kind]
        p = ap.synth.lasso_problem(0, m, n) if kind == "dense" else ap.synth.sparse_lasso_problem(0, m, n, density)
        D, s = p["D"], p["s"]
        g = np.asarray(D.T @ s).reshape(-1)
        run = dict(domaxiters=1, maxiters=args.iters)
        lams = float(np.max(np.abs(g))) * np.logspace(-0.1, -2.0, 10)  # the lasso's path: groups live and die under it too
        with limit(f"create, the {kind} object", 300):
            obj = ap.LassoMulti(D, s, lams) if kind == "dense" else ap.SparseLassoMulti(D, s, lams)
        try:
            legs = [("ungrouped", None)] + [(f"groups of {p_g}", p_g) for p_g in GROUPS]
            for name, p_g in legs:
                sizes = None if p_g is None else np.full(n // p_g, p_g, dtype=np.int64)
                with limit(f"{kind}, ten fits, {name}", 180):
                    obj.set_groups(sizes)
                    us, lo, hi = per_iter_us(lambda: obj.run(**run)["runtime"], args.iters, args.reps)
                emit(kind=kind, m=m, n=n, leg=f"ten fits in one object, {name}", us_per_iter=us, us_min=lo, us_max=hi)
        finally:
            obj.close()
        with limit(f"create, the {kind} grouplasso engine", 300):
            eng = ap.Engine(L.PROB_LASSO, D=D, s=s, lam=0.1 * float(np.max(np.abs(g))))
        try:
            eng.set_profiling(False)
            kw = dict(domaxiters=1, record_history=0, maxiters=args.iters)
            for p_g in GROUPS:
                with limit(f"{kind}, ten runs of the grouplasso engine, groups of {p_g}", 300):
                    eng.set_groups(np.full(n // p_g, p_g, dtype=np.int64))
                    us, lo, hi = per_iter_us(lambda: sum(eng.run(**kw).runtime_s for _ in range(10)), args.iters, args.reps)
                    xs = eng.info()["xsolve_used"]
                ten = next(r for r in rows if r["kind"] == kind and r["leg"] == f"ten fits in one object, groups of {p_g}")
                emit(kind=kind, m=m, n=n, leg=f"ten runs of the grouplasso engine, groups of {p_g}", xsolve=xs, us_per_iter=us,
                     us_min=lo, us_max=hi, ratio_to_one_object=round(us / ten["us_per_iter"], 2))
        finally:
            eng.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
