"""Per-iteration cost of the loss family of the LAD and Huber engines next to the default engines, measured
as profiles/penalty_bench.py measures the lasso's penalty family: the loop's own runtime (two forced run lengths, the
difference divided by the difference in iterations) and the kernels' time by class (HIP events around every 4th launch,
in runs of their own), both legs of a pair in one process.  Pairs: LAD at the defaults against quantile (tau = 0.9) with
weights; Huber at delta = 1 against delta = 0.5 with weights.  Shapes: one tall one (two passes over D per iteration)
and one that takes the one-pass kernel under nodualerror (n <= 448, at least 48 MB).

    python profiles/loss_bench.py [--tall 40000x2000] [--onepass 60000x400] [--reps 5] [--legs all|default] [--out file.json]
prints one JSON line per case.  --legs default times the default LAD legs alone (one process per build: the figure to
set next to another build's); on a build without admm_engine_set_loss only those run.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402


def measure(eng, L, args, kw):
    eng.set_profiling(False)
    eng.run(maxiters=args.short, **kw)  # warm-up
    per = []
    for _ in range(args.reps):
        t_short = eng.run(maxiters=args.short, **kw).runtime_s
        t_long = eng.run(maxiters=args.long, **kw).runtime_s
        per.append((t_long - t_short) / (args.long - args.short) * 1e6)
    kinds = (L.K_XSOLVE, L.K_GEMV_N, L.K_PROX, L.K_GEMV_T, L.K_FINALIZE)
    eng.set_profiling(list(kinds), stride=4)
    ker, prox = [], []
    for _ in range(args.reps):
        eng.run(maxiters=args.long, **kw)
        tot = 0.0
        for which in kinds:
            ms, cnt = eng.kernel_time(which)
            per_launch = ms / max(cnt, 1) * 1e3
            launches = cnt * 4 / args.long  # launches of the class per iteration (every 4th was timed)
            tot += per_launch * launches
            if which == L.K_PROX:
                prox.append(per_launch)
        ker.append(tot)
    eng.set_profiling(False)
    r = lambda v: round(float(v), 2)
    return dict(us_per_iter=r(np.median(per)), us_min=r(np.min(per)), us_max=r(np.max(per)),
                kernels_us=r(np.median(ker)), kernels_us_min=r(np.min(ker)), kernels_us_max=r(np.max(ker)),
                element_update_us=r(np.median(prox)), element_update_us_min=r(np.min(prox)),
                element_update_us_max=r(np.max(prox)))


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--tall", default="40000x2000")
    a.add_argument("--onepass", default="60000x400")
    a.add_argument("--reps", type=int, default=5)
    a.add_argument("--short", type=int, default=50)
    a.add_argument("--long", type=int, default=250)
    a.add_argument("--legs", default="all", choices=["all", "default"])
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    L = ap._lib
    rows = []
    for label, shape, kw in (("tall", args.tall, dict(domaxiters=1, record_history=0)),
                             ("onepass", args.onepass, dict(domaxiters=1, record_history=0, nodualerror=1))):
        m, n = (int(v) for v in shape.split("x"))
        p = ap.synth.lad_problem(0, m, n)
        w = np.random.default_rng(1).uniform(0.5, 2.0, m)
        for code, name in ((L.PROB_LAD, "lad"), (L.PROB_HUBERFIT, "huberfit")):
            if args.legs == "default" and name != "lad":
                continue
            eng = ap.Engine(code, D=p["D"], s=p["s"])
            try:
                legs = [(f"{name}, defaults", None)]
                if args.legs == "all" and hasattr(eng, "set_loss"):
                    legs.append(("quantile 0.9 + weights", dict(weights=w, slopes=(0.9, 0.1))) if name == "lad" else
                                ("huber delta 0.5 + weights", dict(weights=w, delta=0.5)))
                for case, loss in legs:
                    if loss is not None:
                        eng.set_loss(**loss)
                    rows.append(dict(shape=label, m=m, n=n, case=case, reps=args.reps, **measure(eng, L, args, kw)))
                    print(json.dumps(rows[-1]), flush=True)
            finally:
                eng.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
