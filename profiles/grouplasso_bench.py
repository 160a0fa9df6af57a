"""Per-iteration cost of group lasso next to plain lasso on one engine: the loop's own runtime (two forced run lengths,
the difference divided by the difference in iterations, as profiles/svm_logistic_bench.py) and the element update's
kernel time (HIP events around its launch, every 4th iteration, in a run of its own), at 12000 x 10000: the loop costs
what the headline's does and setup stays short.  Cases: plain lasso, groups of 10, groups of 1000.

    python profiles/grouplasso_bench.py [--shape 12000x10000] [--groups 10 1000] [--reps 5] [--out file.json]
prints one JSON line per case.  On a build without admm_engine_set_groups only the plain case runs (the parent's figure).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--shape", default="12000x10000")
    a.add_argument("--groups", nargs="*", type=int, default=[10, 1000])
    a.add_argument("--reps", type=int, default=5)
    a.add_argument("--short", type=int, default=100)
    a.add_argument("--long", type=int, default=500)
    a.add_argument("--xsolve", default="auto")
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    L = ap._lib
    m, n = (int(v) for v in args.shape.split("x"))
    p = ap.synth.lasso_problem(0, m, n)
    xs = {"auto": L.XSOLVE_AUTO, "trsv": L.XSOLVE_TRSV, "inverse": L.XSOLVE_INVERSE}[args.xsolve]
    eng = ap.Engine(L.PROB_LASSO, D=p["D"], s=p["s"], lam=p["lam"], xsolve=xs)
    rows = []
    try:
        cases = [("plain", None)]
        if hasattr(eng, "set_groups"):
            cases += [(f"groups of {g}", g) for g in args.groups]
        for name, g in cases:
            if g is not None:
                sizes = [g] * (n // g) + ([n % g] if n % g else [])
                eng.set_groups(sizes)
            kw = dict(domaxiters=1, record_history=0)
            eng.set_profiling(False)
            eng.run(maxiters=args.short, **kw)  # warm-up
            per = []
            for _ in range(args.reps):
                t_short = eng.run(maxiters=args.short, **kw).runtime_s
                t_long = eng.run(maxiters=args.long, **kw).runtime_s
                per.append((t_long - t_short) / (args.long - args.short) * 1e6)
            eng.set_profiling([L.K_PROX, L.K_XSOLVE], stride=4)
            prox, xsol = [], []
            for _ in range(args.reps):
                eng.run(maxiters=args.long, **kw)
                for which, out in ((L.K_PROX, prox), (L.K_XSOLVE, xsol)):
                    ms, cnt = eng.kernel_time(which)
                    out.append(ms / max(cnt, 1) * 1e3)
            info = eng.info()
            rows.append(dict(m=m, n=n, case=name, xsolve=info["xsolve_used"], us_per_iter=round(float(np.median(per)), 2),
                             us_min=round(float(np.min(per)), 2), us_max=round(float(np.max(per)), 2),
                             element_update_us=round(float(np.median(prox)), 2),
                             element_update_us_min=round(float(np.min(prox)), 2),
                             element_update_us_max=round(float(np.max(prox)), 2),
                             xsolve_us=round(float(np.median(xsol)), 2), reps=args.reps))
            print(json.dumps(rows[-1]), flush=True)
    finally:
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
