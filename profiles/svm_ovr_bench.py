"""Per-iteration cost of linearsvm_ovr against K sequential linearsvm runs, at MNIST's full size (60000 x 400,
synthetic pixels: synth.mnist_like_problem), K = 1, 10, 20, domaxiters = 1.

The one-vs-rest loop is timed with HIP events on its own stream (admm_svm_ovr_run's runtime): two forced run lengths
per repetition, and the per-iteration cost is their difference divided by the difference in iterations, so the
start-up pass D'(z0 - u0) and the first poll drop out.  The sequential side is the per-class engine's own loop runtime
over its forced 1000 iterations, same process, same device, classes one after the other.

    python profiles/svm_ovr_bench.py [--m 60000] [--n 400] [--reps 5] [--out file.json]
prints one JSON line per K: us per iteration for both, their ratio, and bytes of D read per iteration / time.
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
    a.add_argument("--m", type=int, default=60000)
    a.add_argument("--n", type=int, default=400)
    a.add_argument("--reps", type=int, default=5)
    a.add_argument("--short", type=int, default=50)
    a.add_argument("--long", type=int, default=250)
    a.add_argument("--ks", type=int, nargs="+", default=[1, 10, 20])
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    m, n = args.m, args.n
    p = ap.synth.mnist_like_problem(seed=1, m=m, n=n)
    rng = np.random.default_rng(5)
    labels = rng.integers(0, 10, size=m).astype(np.float64)
    kmax = max(args.ks)
    classes = np.arange(kmax) % 10.0
    losses = ["hinge" if c < 10 else "01" for c in range(kmax)]  # mnistsvm.m:88-102: ten digits, both losses
    ELL = ap.solvers.ovr_label_matrix(labels, classes)
    x0, z0, u0 = rng.random((n, kmax)), rng.random((m, kmax)), rng.random((m, kmax))
    chunk = ap._lib.load().admm_svm_ovr_chunk()

    # ---- the parent path: one engine per class, classes one after the other
    seq_us = []
    for c in range(kmax):
        r = ap.linearsvm(p["D"], ELL[:, c], p["C"], dict(domaxiters=1, lossfunction=losses[c], x0=x0[:, c],
                                                        z0=z0[:, c], u0=u0[:, c], record_history=0))
        assert r["steps"] == 1000
        seq_us.append(r["runtime"] / r["steps"] * 1e6)

    rows = []
    for K in args.ks:
        obj = ap.SvmOvr(p["D"], np.asfortranarray(ELL[:, :K]), p["C"], losses[:K])
        kw = dict(domaxiters=1, x0=np.asfortranarray(x0[:, :K]), z0=np.asfortranarray(z0[:, :K]),
                  u0=np.asfortranarray(u0[:, :K]))
        try:
            obj.run(maxiters=args.short, **kw)  # warm-up: code objects, clocks, caches
            per = []
            for _ in range(args.reps):
                t_short = obj.run(maxiters=args.short, **kw)["runtime"]
                t_long = obj.run(maxiters=args.long, **kw)["runtime"]
                per.append((t_long - t_short) / (args.long - args.short) * 1e6)
        finally:
            obj.close()
        ovr = float(np.median(per))
        seq = float(np.sum(seq_us[:K]))
        passes = -(-K // chunk)
        rows.append(dict(m=m, n=n, K=K, chunk=chunk, passes_per_iter=passes, ovr_us_per_iter=round(ovr, 2),
                         ovr_us_min=round(float(np.min(per)), 2), ovr_us_max=round(float(np.max(per)), 2),
                         sequential_us_per_iter=round(seq, 2), speedup=round(seq / ovr, 3),
                         ovr_read_TBps=round(passes * 8.0 * m * n / (ovr * 1e-6) / 1e12, 3),
                         sequential_us_per_class=round(float(np.mean(seq_us[:K])), 2), reps=args.reps))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
