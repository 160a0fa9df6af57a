"""Per-iteration cost of the logistic loss next to the hinge: the single-class engine (`linearsvm`, its forced 1000
iterations, the loop's own runtime) and the ten-class one-vs-rest pass (`admm_svm_ovr_run`, two forced run lengths, the
difference divided by the difference in iterations, as profiles/svm_ovr_bench.py), at 6000 x 400 and 60000 x 400
(synthetic pixels: synth.mnist_like_problem).

    python profiles/svm_logistic_bench.py [--shapes 6000x400 60000x400] [--reps 5] [--out file.json]
prints one JSON line per shape and loss.
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
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    rows = []
    for shape in args.shapes:
        m, n = (int(v) for v in shape.split("x"))
        p = ap.synth.mnist_like_problem(seed=1, m=m, n=n)
        rng = np.random.default_rng(5)
        labels = rng.integers(0, 10, size=m).astype(np.float64)
        ELL = ap.solvers.ovr_label_matrix(labels, np.arange(10.0))
        x0, z0, u0 = rng.random((n, 10)), rng.random((m, 10)), rng.random((m, 10))
        for loss in ("hinge", "logistic"):
            single = []
            for _ in range(args.reps):
                r = ap.linearsvm(p["D"], ELL[:, 0], p["C"], dict(domaxiters=1, lossfunction=loss, x0=x0[:, 0], z0=z0[:, 0],
                                                                u0=u0[:, 0], record_history=0))
                assert r["steps"] == 1000
                single.append(r["runtime"] / r["steps"] * 1e6)
            obj = ap.SvmOvr(p["D"], ELL, p["C"], [loss] * 10)
            kw = dict(domaxiters=1, x0=np.asfortranarray(x0), z0=np.asfortranarray(z0), u0=np.asfortranarray(u0))
            try:
                obj.run(maxiters=args.short, **kw)  # warm-up
                per = []
                for _ in range(args.reps):
                    t_short = obj.run(maxiters=args.short, **kw)["runtime"]
                    t_long = obj.run(maxiters=args.long, **kw)["runtime"]
                    per.append((t_long - t_short) / (args.long - args.short) * 1e6)
            finally:
                obj.close()
            ten = float(np.median(per))
            rows.append(dict(m=m, n=n, loss=loss, single_us_per_iter=round(float(np.median(single)), 2),
                             single_us_min=round(float(np.min(single)), 2), single_us_max=round(float(np.max(single)), 2),
                             ten_class_us_per_iter=round(ten, 2), ten_us_min=round(float(np.min(per)), 2),
                             ten_us_max=round(float(np.max(per)), 2),
                             ten_class_read_TBps=round(8.0 * m * n / (ten * 1e-6) / 1e12, 3), reps=args.reps))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
