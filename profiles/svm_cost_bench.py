"""Per-iteration cost of the linear SVM's costs and of the squared hinge, both legs in one process: the default hinge
against hinge with weights and class costs, and 'sqhinge' against hinge, for one class (the engine's own loop: the
two-launch form at 6000 x 400, the one-pass form at 60000 x 400) and for the ten-class one-vs-rest pass, on synthetic
pixels (synth.mnist_like_problem), domaxiters = 1.

The single-class legs are the engine's loop runtime over its forced 1000 iterations (as profiles/svm_ovr_bench.py's
sequential side); the one-vs-rest legs are timed with HIP events on the object's stream, two forced run lengths per
repetition, per-iteration cost = difference of the runtimes / difference of the iterations.  The legs alternate inside
every repetition, so drift of the clocks falls on all of them.

    python profiles/svm_cost_bench.py [--shapes 6000x400 60000x400] [--reps 5] [--only default] [--out file.json]
prints one JSON line per shape and leg: median, min and max us per iteration.  --only default runs the default hinge leg
alone (the leg to compare between two builds, each in a process of its own).
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
    a.add_argument("--shapes", nargs="+", default=["6000x400", "60000x400"])
    a.add_argument("--reps", type=int, default=5)
    a.add_argument("--short", type=int, default=50)
    a.add_argument("--long", type=int, default=250)
    a.add_argument("--only", default=None, help="run this leg alone (default, costs, sqhinge)")
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    legs = {"default": dict(lossfunction="hinge"), "costs": dict(lossfunction="hinge", weighted=True),
            "sqhinge": dict(lossfunction="sqhinge")}
    if args.only:
        legs = {args.only: legs[args.only]}
    rows = []
    for shape in args.shapes:
        m, n = (int(v) for v in shape.split("x"))
        p = ap.synth.mnist_like_problem(seed=1, m=m, n=n)
        rng = np.random.default_rng(5)
        labels = rng.integers(0, 10, size=m).astype(np.float64)
        w = rng.uniform(0.25, 4.0, m)
        K = 10
        classes = np.arange(float(K))
        ELL = ap.solvers.ovr_label_matrix(labels, classes)
        x0, z0, u0 = (np.asfortranarray(rng.random((r, K))) for r in (n, m, m))
        single = {k: [] for k in legs}
        ovr = {k: [] for k in legs}
        objs = {}
        try:
            for k, leg in legs.items():
                objs[k] = ap.SvmOvr(p["D"], ELL, p["C"], [leg["lossfunction"]] * K)
                if leg.get("weighted"):
                    objs[k].set_cost(w, np.array([[m / (2.0 * np.sum(ELL[:, c] > 0)), m / (2.0 * np.sum(ELL[:, c] < 0))]
                                                  for c in range(K)]))
                objs[k].run(maxiters=args.short, domaxiters=1, x0=x0, z0=z0, u0=u0)  # warm-up
            for _ in range(args.reps):
                for k, leg in legs.items():
                    o = dict(domaxiters=1, lossfunction=leg["lossfunction"], x0=x0[:, 0], z0=z0[:, 0], u0=u0[:, 0],
                             record_history=0)
                    if leg.get("weighted"):
                        o.update(weights=w, classcost="balanced")
                    r = ap.linearsvm(p["D"], ELL[:, 0], p["C"], o)
                    assert r["steps"] == 1000
                    single[k].append(r["runtime"] / r["steps"] * 1e6)
                    kw = dict(domaxiters=1, x0=x0, z0=z0, u0=u0)
                    t_short = objs[k].run(maxiters=args.short, **kw)["runtime"]
                    t_long = objs[k].run(maxiters=args.long, **kw)["runtime"]
                    ovr[k].append((t_long - t_short) / (args.long - args.short) * 1e6)
        finally:
            for obj in objs.values():
                obj.close()
        for k in legs:
            for what, per in (("single", single[k]), ("ovr10", ovr[k])):
                rows.append(dict(m=m, n=n, leg=k, what=what, us_per_iter=round(float(np.median(per)), 2),
                                 us_min=round(float(np.min(per)), 2), us_max=round(float(np.max(per)), 2), reps=args.reps))
                print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
