"""Covariance selection over K lambda values: K = 1, 10, 64 and 256 fits through the multi-fit object
(one workgroup per fit, the whole iteration in one kernel) against K sequential runs of the single-fit
``covarianceselection`` engine -- one engine per lambda, one after the other -- on the same S in the same process, at
n = 32, 64 and 96.

Per leg: microseconds per iteration of the whole leg (all K fits advance one iteration) from the loops' own event-timed
runtimes over a forced run length (domaxiters; the median of --reps runs with their spread), and the ratios
object / sequential and object(K) / object(1).  The lambda grid is lambda_max * logspace(0, -2, K).  Every GPU step runs
under its own time limit: a watchdog ends the process with status 124 if a step overruns it.

    python profiles/covsel_multi_bench.py [--sizes 32,64,96] [--fits 1,10,64,256] [--iters 40] [--reps 5] [--out f.json]
prints one JSON line per leg.
"""
import argparse
import json
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402


class limit:
    """a GPU step with a time limit of its own: the process ends (status 124) when the step overruns it"""

    def __init__(self, what, seconds):
        self.what, self.seconds = what, seconds

    def __enter__(self):
        def overrun():
            sys.stderr.write(f"time limit: {self.what} ran longer than {self.seconds} s\n")
            sys.stderr.flush()
            os._exit(124)
        self.timer = threading.Timer(self.seconds, overrun)
        self.timer.daemon = True
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()
        return False


def spread(ts):
    return round(float(np.median(ts)), 2), round(float(min(ts)), 2), round(float(max(ts)), 2)


def problem(n, seed=7):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    Cov = G @ G.T / n + 0.5 * np.eye(n)
    D = rng.standard_normal((8 * n, n)) @ np.linalg.cholesky(Cov).T
    S = np.atleast_2d(np.cov(D, rowvar=False))
    return np.asfortranarray(0.5 * (S + S.T))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="32,64,96")
    p.add_argument("--fits", default="1,10,64,256")
    p.add_argument("--iters", type=int, default=40)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    ap._lib.require_device()
    loop = dict(maxiters=a.iters, domaxiters=1, check_every=a.iters)
    lines = []
    for n in (int(v) for v in a.sizes.split(",")):
        S = problem(n)
        off = np.abs(S - np.diag(np.diag(S)))
        lmax = float(off.max())
        one_us = None
        for K in (int(v) for v in a.fits.split(",")):
            lams = lmax * np.logspace(0.0, -2.0, K) if K > 1 else np.array([0.3 * lmax])
            with limit(f"object n={n} K={K}", 120):
                obj = ap.CovselMulti(lams, S=S)
                try:
                    run = lambda: obj.run(**loop)["runtime"] / a.iters * 1e6
                    run()  # warm-up
                    multi = spread([run() for _ in range(a.reps)])
                    sweeps = float(np.mean(obj.run(**loop)["jacobi_sweeps"])) / a.iters
                finally:
                    obj.close()
            if K == 1:
                one_us = multi[0]

            def sequential():
                total = 0.0
                for lam in lams:
                    minx, minz, _ = ap.getproxops("covarianceselection", {"S": S, "lambda": float(lam)})
                    try:
                        o = dict(A=1, B=-1, c=0, m=n, nA=n, nB=n, record_history=0, **loop)
                        total += ap.admm(minx, minz, o)["runtime"]
                    finally:
                        minx.problem.engine.close()
                return total / a.iters * 1e6
            with limit(f"sequential n={n} K={K}", 400):
                sequential()  # warm-up
                seq = spread([sequential() for _ in range(a.reps)])
            line = dict(n=n, K=K, iters=a.iters, reps=a.reps, object_us_per_iter=multi[0], object_min_max=multi[1:],
                        sequential_us_per_iter=seq[0], sequential_min_max=seq[1:],
                        object_over_sequential=round(multi[0] / seq[0], 4),
                        object_over_one_fit=round(multi[0] / one_us, 3) if one_us else None,
                        sweeps_per_x_update=round(sweeps, 2))
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
