"""One SHA-256 per case over the iterates and the scalar histories of short seeded runs that reach every launcher of an
element-update family (loop_kernels.h: ProxFamily): the penalised and the sparse-group lasso in the one-launch tail with
the finalize in the launch (300 x 200), deferred behind the x-solve's partial rows (2000 x 1600) and in launch_prox's
place (weak fast ADMM); the loss family in prox_kernel, in the tail (nodualerror) and in the one-pass kernel
(14080 x 448); the SVM's cost form in the two-launch unwrapped iteration and in the generic kernels (fast ADMM).

Two builds that compute the same bits print the same lines on one machine; the hashes are no portable constant.

    python profiles/family_bits.py [--root DIR]
--root: the tree whose package and library are loaded (default: the tree this file is in).
"""
import argparse
import hashlib
import os
import sys

import numpy as np

KEYS = ("steps", "xopt", "zopt", "uopt", "xvals", "zvals", "uvals", "vvals", "uhatvals", "pnorm", "dnorm", "perr", "derr",
        "objevals", "Hnormsq", "avals", "dvals", "restarted")


def digest(res):
    h = hashlib.sha256()
    for k in KEYS:
        if k in res and res[k] is not None:
            h.update(k.encode())
            h.update(np.ascontiguousarray(np.asarray(res[k], dtype=np.float64)).tobytes())
    return h.hexdigest()


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = a.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import admm_project_amd as ap

    ap._lib.require_device()
    forced = dict(objevals=1, maxiters=12, domaxiters=1)
    strong, weak = dict(fast=1, fasttype="strong"), dict(fast=1, fasttype="weak")

    def show(name, res):
        print(f"{digest(res)}  {name}", flush=True)

    # ---- the lasso's penalty family, without and with groups
    for m, n, sizes in ((300, 200, [1, 7, 64, 100, 28]), (2000, 1600, [3, 125, 130, 442, 500, 400])):
        p = ap.synth.lasso_problem(7, m, n)
        rng = np.random.default_rng(n)
        w = rng.uniform(0.5, 2.0, n)
        w[n // 2] = 0.0
        gw = np.sqrt(np.asarray(sizes, dtype=np.float64))
        runs = [("plain", {}), ("strong", strong)] + ([("weak", weak)] if n == 200 else [])
        for tag, extra in runs:
            o = dict(forced, **extra)
            show(f"penalised lasso {m}x{n} {tag}",
                 ap.lasso(p["D"], p["s"], p["lam"], dict(o, l1weights=w, ridge=0.5, nonnegative=1)))
            show(f"sparse-group lasso {m}x{n} {tag}",
                 ap.grouplasso(p["D"], p["s"], p["lam"], sizes, dict(o, l1=0.5 * p["lam"], ridge=0.25, groupweights=gw)))
    # ---- the loss family: prox_kernel, the tail under nodualerror, the one-pass kernel
    p = ap.synth.lad_problem(3, 300, 40)
    w = np.random.default_rng(5).uniform(0.5, 2.0, 300)
    w[::17] = 0.0
    for tag, extra in (("", {}), (" nodualerror", dict(nodualerror=1))):
        o = dict(forced, **extra)
        show(f"LAD quantile 300x40{tag}", ap.lad(p["D"], p["s"], dict(o, weights=w, slopes=(0.9, 0.1))))
        show(f"Huber 300x40{tag}", ap.huberfit(p["D"], p["s"], dict(o, weights=w, slopes=(1.5, 0.5), delta=0.5)))
    p = ap.synth.lad_problem(4, 14080, 448)
    w = np.random.default_rng(6).uniform(0.5, 2.0, 14080)
    show("LAD quantile 14080x448 nodualerror (one pass)",
         ap.lad(p["D"], p["s"], dict(forced, nodualerror=1, weights=w, slopes=(0.9, 0.1))))
    # ---- the SVM's cost form: the two-launch unwrapped iteration, and the generic kernels under fast ADMM
    p = ap.synth.mnist_like_problem(seed=3, m=700, n=57)
    w = np.random.default_rng(8).uniform(0.25, 4.0, 700)
    w[::17] = 0.0
    start = dict(x0=p["x0"], z0=p["z0"], u0=p["u0"])
    for loss in ("hinge", "sqhinge", "logistic"):
        o = dict(forced, lossfunction=loss, weights=w, classcost=(2.0, 0.5), **start)
        show(f"SVM costs {loss} 700x57 unwrapped", ap.linearsvm(p["D"], p["ell"], p["C"], o))
        show(f"SVM costs {loss} 700x57 strong", ap.linearsvm(p["D"], p["ell"], p["C"], dict(o, **strong)))
        show(f"SVM costs {loss} 700x57 weak", ap.linearsvm(p["D"], p["ell"], p["C"], dict(o, **weak)))


if __name__ == "__main__":
    main()
