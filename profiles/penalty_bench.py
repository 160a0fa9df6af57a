"""Per-iteration cost of the lasso's penalty family next to plain lasso on one engine, measured as
profiles/grouplasso_bench.py measures group lasso: the loop's own runtime (two forced run lengths, the difference divided
by the difference in iterations) and the element update's kernel time (HIP events around its launch, every 4th
iteration, in a run of its own), at 12000 x 10000.  Cases: plain lasso; l1 weights + ridge + sign constraint (the
elementwise kernel); sparse-group with groups of 10, sqrt(10) weights, l1 > 0 and a ridge term (the grouped kernel's
penalised instantiation); plain group lasso with the same groups for comparison.

    python profiles/penalty_bench.py [--shape 12000x10000] [--group 10] [--reps 5] [--out file.json]
prints one JSON line per case.  On a build without admm_engine_set_penalty only the plain case runs (the parent's figure).
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
    a.add_argument("--group", type=int, default=10)
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
        g = args.group
        sizes = [g] * (n // g) + ([n % g] if n % g else [])
        w = np.random.default_rng(1).uniform(0.5, 2.0, n)
        cases = [("plain", None)]
        if hasattr(eng, "set_penalty"):
            cases += [("weights + ridge + sign", "elem"), (f"group lasso, groups of {g}", "group"),
                      (f"sparse-group, groups of {g}", "sparsegroup")]
        for name, kind in cases:
            if kind == "elem":
                eng.set_penalty(w, 0.5, 1)
            elif kind == "group":
                eng.set_penalty(None)
                eng.set_groups(sizes, np.sqrt(np.asarray(sizes, dtype=np.float64)))
            elif kind == "sparsegroup":
                eng.set_penalty(w, 0.5, 0, 0.5 * p["lam"])
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
