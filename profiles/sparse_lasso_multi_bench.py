"""The lasso over several lambda values on a sparse design matrix: ten, five and one lambda through the
multi-fit object (lock-step CG over the ten-wide sparse product) against ten runs of ``lasso``'s sparse engine (q35: one
fit per engine, one-column SpMV) on the same matrix in the same process, at 100000 x 10000 with density 1 % and 0.1 %.

Per leg: the loop's own event-timed runtime (a forced run length, domaxiters) as the median of --reps runs with their
spread, microseconds per lock-step inner iteration (runtime / the largest per-fit inner count), and "ten for the price of
how many": the K = 10 run over the mean single-engine run, and over the K = 1 run of the object itself.

    python profiles/sparse_lasso_multi_bench.py [--shape 100000x10000] [--iters 5] [--reps 3] [--cg-maxit 30] [--out f.json]
prints one JSON line per leg.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402


def timed(obj, args, **more):
    kw = dict(domaxiters=1, maxiters=args.iters, cg_maxit=args.cg_maxit, **more)
    obj.run(**kw)  # warm-up
    runs = [obj.run(**kw) for _ in range(args.reps)]
    ts = [r["runtime"] for r in runs]
    return float(np.median(ts)), float(max(ts) - min(ts)), runs[-1]


def multi(D, s, lams, args):
    obj = ap.SparseLassoMulti(D, s, lams)
    try:
        t, spread, last = timed(obj, args)
    finally:
        obj.close()
    inner = int(last["cg_iters_total"].max())
    return dict(ms=t * 1e3, spread_ms=spread * 1e3, inner=inner, us_per_inner=t / max(inner, 1) * 1e6,
                capped=[int(v) for v in last["cg_capped_updates"]])


def engine(D, s, lam, args):
    """one lambda on lasso's sparse engine: (loop ms, inner iterations)"""
    L = ap._lib
    eng = ap.Engine(L.PROB_LASSO, D=D, s=s, lam=float(lam), cg_maxit=args.cg_maxit)
    try:
        kw = dict(domaxiters=1, record_history=0, maxiters=args.iters)
        eng.set_profiling(False)
        eng.run(**kw)  # warm-up
        ts = [eng.run(**kw).runtime_s for _ in range(args.reps)]
        return float(np.median(ts)) * 1e3, int(eng.fetch(L.F_CG_ITERS, 2)[0])
    finally:
        eng.close()


def leg(name, p, args):
    D, s = p["D"], p["s"]
    lmax = float(np.max(np.abs(D.T @ s)))
    lams = lmax * np.logspace(0.0, -2.0, 10)
    ten, five, one = multi(D, s, lams, args), multi(D, s, lams[::2], args), multi(D, s, lams[5:6], args)
    singles = [engine(D, s, lam, args) for lam in lams]
    ms10 = float(sum(t for t, _ in singles))
    inner10 = int(sum(i for _, i in singles))
    r = lambda v: round(float(v), 2)
    row = dict(leg=name, m=D.shape[0], n=D.shape[1], nnz=int(D.nnz), chunk=ap.SparseLassoMulti.chunk(),
               admm_iters=args.iters, cg_maxit=args.cg_maxit, reps=args.reps,
               ms_ten=r(ten["ms"]), spread_ten_ms=r(ten["spread_ms"]), inner_ten=ten["inner"],
               us_per_inner_ten=r(ten["us_per_inner"]),
               ms_five=r(five["ms"]), inner_five=five["inner"], us_per_inner_five=r(five["us_per_inner"]),
               ms_one=r(one["ms"]), inner_one=one["inner"], us_per_inner_one=r(one["us_per_inner"]),
               ms_ten_engines=r(ms10), inner_ten_engines=inner10, us_per_inner_engine=r(ms10 * 1e3 / max(inner10, 1)),
               ten_for_the_price_of_engines=r(ten["ms"] / (ms10 / 10.0)),
               ten_for_the_price_of_own_single=r(ten["ms"] / one["ms"]), speedup_over_ten_engines=r(ms10 / ten["ms"]),
               capped_updates_ten=ten["capped"])
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
        rows.append(leg(name, ap.synth.sparse_lasso_problem(seed, m, n, density), args))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
