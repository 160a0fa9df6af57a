"""The one-vs-rest linear SVM on a sparse design matrix: K = 1, 5, 10 classes in one object against K
runs of the K = 1 object in the same process, at 100000 x 10000 with density 1 % and 0.1 %.

Per leg: the loop's own event-timed runtime (a forced run length), microseconds per ADMM iteration and per lock-step
inner iteration (runtime / the largest per-class inner count), and the bytes one inner iteration moves by the derived
model of EXPERIMENTS.md -- 24 B per nonzero once per chunk plus the multi-vector traffic -- per second.

    python profiles/sparse_svm_bench.py [--shape 100000x10000] [--iters 5] [--reps 3] [--cg-maxit 30] [--out file.json]
prints one JSON line per leg.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402


def timed(obj, args, z0, u0):
    kw = dict(domaxiters=1, maxiters=args.iters, cg_maxit=args.cg_maxit, z0=z0, u0=u0)
    obj.run(**kw)  # warm-up
    runs = [obj.run(**kw) for _ in range(args.reps)]
    t = float(np.median([r["runtime"] for r in runs]))
    return t, runs[-1]


def leg(name, p, K, args):
    D, m, n = p["D"], p["D"].shape[0], p["D"].shape[1]
    ELL = np.asfortranarray(np.where(p["labels"][:, None] == np.arange(K)[None, :], 1.0, -1.0))
    rng = np.random.default_rng(3)
    z0, u0 = np.asfortranarray(rng.random((m, K))), np.asfortranarray(rng.random((m, K)))
    obj = ap.SparseSvmOvr(D, ELL, p["C"], ["hinge"] * K)
    try:
        t, last = timed(obj, args, z0, u0)
    finally:
        obj.close()
    t1 = 0.0  # the same K classes as K runs of the one-class object
    for c in range(K):
        one = ap.SparseSvmOvr(D, ELL[:, c:c + 1], p["C"], ["hinge"])
        try:
            t1 += timed(one, args, z0[:, c:c + 1], u0[:, c:c + 1])[0]
        finally:
            one.close()
    inner = int(last["cg_iters_total"].max())
    kc = ap.SparseSvmOvr.chunk()
    chunks = -(-K // kc)
    # two products: 12 B per nonzero and the row starts each, P / T read and T / Q written; dot, update, direction: 11 n
    moved = chunks * (24.0 * D.nnz + 8.0 * (m + n + 2)) + 8.0 * kc * chunks * (2 * m + 2 * n + 11 * n)
    row = dict(leg=name, m=m, n=n, nnz=int(D.nnz), K=K, chunk=kc, admm_iters=args.iters, inner_iters=inner,
               ms_K_classes=round(t * 1e3, 2), ms_K_single_runs=round(t1 * 1e3, 2), speedup=round(t1 / t, 2),
               us_per_admm_iter=round(t / args.iters * 1e6, 1), us_per_inner_iter=round(t / max(inner, 1) * 1e6, 1),
               model_bytes_per_inner_iter=int(moved), model_tb_per_s=round(moved / (t / max(inner, 1)) / 1e12, 3),
               capped_updates=[int(v) for v in last["cg_capped_updates"]], reps=args.reps)
    print(json.dumps(row), flush=True)
    return row


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--shape", default="100000x10000")
    a.add_argument("--iters", type=int, default=5)
    a.add_argument("--reps", type=int, default=3)
    a.add_argument("--cg-maxit", type=int, default=30)
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    m, n = (int(v) for v in args.shape.split("x"))
    rows = []
    for name, density, seed in (("1 %", 0.01, 0), ("0.1 %", 0.001, 1)):
        p = ap.synth.sparse_svm_problem(seed, m, n, density, classes=10)
        for K in (1, 5, 10):
            rows.append(leg(f"{name} K={K}", p, K, args))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
