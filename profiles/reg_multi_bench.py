"""Multi-fit quantile regression against the single engine: microseconds per iteration.

    python profiles/reg_multi_bench.py [--iters 200] [--repeats 5] [--shapes 6000x400,60000x400]

All legs run in one process, on one D per shape (synth.quantile_problem):
  leg 1  K = 1, 5, 10 quantiles through admm_reg_multi (RegMulti), domaxiters = 1
  leg 2  the existing ADMM_PROB_LAD engine on one quantile with nodualerror = 1, domaxiters = 1
Every leg is timed by its own loop timer (HIP events around the loop) over --iters iterations after one warm-up run,
--repeats times; the median and the spread (min .. max) are reported, and the ratio K-fit / (K x single).  Prints one JSON
line per shape.  No figure here is asserted anywhere."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import admm_project_amd as ap  # noqa: E402


def _stats(us):
    us = sorted(us)
    return dict(median=round(us[len(us) // 2], 2), min=round(us[0], 2), max=round(us[-1], 2))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--shapes", default="6000x400,60000x400")
    a = p.parse_args()
    L = ap._lib
    ap._lib.require_device()
    for shape in a.shapes.split(","):
        m, n = (int(v) for v in shape.split("x"))
        prob = ap.synth.quantile_problem(0, m, n)
        D, s = prob["D"], prob["s"]
        out = dict(shape=[m, n], iters=a.iters, repeats=a.repeats, chunk=ap.RegMulti.chunk())
        eng = ap.Engine(L.PROB_LAD, D=D, s=s)
        try:
            eng.set_loss(None, (0.5, 0.5), 0.0, 1.0)
            run = lambda: eng.run(maxiters=a.iters, domaxiters=1, nodualerror=1, record_history=0)
            run()
            single = [1e6 * run().runtime_s / a.iters for _ in range(a.repeats)]
        finally:
            eng.close()
        out["single_us_per_iter"] = _stats(single)
        for K in (1, 5, 10):
            taus = np.linspace(0.05, 0.95, K) if K > 1 else np.array([0.5])
            obj = ap.RegMulti(D, s, [0] * K, list(taus), list(1.0 - taus))
            try:
                obj.run(maxiters=a.iters, domaxiters=1)
                us = [1e6 * obj.run(maxiters=a.iters, domaxiters=1)["runtime"] / a.iters for _ in range(a.repeats)]
                out[f"multi_K{K}_explicit_map"] = obj.launches()["explicit_map"]
            finally:
                obj.close()
            st = _stats(us)
            out[f"multi_K{K}_us_per_iter"] = st
            out[f"ratio_K{K}_over_Kx_single"] = round(st["median"] / (K * out["single_us_per_iter"]["median"]), 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
