"""Per-iteration cost of isotropic next to anisotropic 2-D total variation on ONE engine (spectral x-update): the loop's
own runtime (two forced run lengths, the difference divided by the difference in iterations, as
profiles/grouplasso_bench.py) and, in runs of their own, the event-timed launch groups -- the x-update and the fused
pixel pass (at 4096 x 4096 the three-launch form: the pixel pass is tv2d_fused_dct_kernel, forward column transform
included; a height that is no power of two, e.g. 4000x4096, takes the four-launch form with tv2d_fused_kernel).  The two
norms alternate inside every repetition, so both see the same machine.

    python profiles/tv2d_iso_bench.py [--shape 4096x4096] [--reps 7] [--short 50] [--long 250] [--cases anisotropic]
                                      [--out file.json]
prints one JSON line per case (--cases anisotropic: that case alone in the process, as a build without the option runs
it).  On a build without admm_engine_set_tv2d_isotropic only the anisotropic case runs (the parent's figure).
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
    a.add_argument("--shape", default="4096x4096")
    a.add_argument("--reps", type=int, default=7)
    a.add_argument("--short", type=int, default=50)
    a.add_argument("--long", type=int, default=250)
    a.add_argument("--rho", type=float, default=1.0)
    a.add_argument("--cases", nargs="*", default=["anisotropic", "isotropic"], choices=["anisotropic", "isotropic"])
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    L = ap._lib
    H, W = (int(v) for v in args.shape.split("x"))
    rng = np.random.default_rng(1)
    img = np.zeros((H, W))
    img[H // 5:H // 2, W // 6:W // 2] = 2.0
    img[H // 3:4 * H // 5, W // 3:5 * W // 6] += 1.0
    img += rng.standard_normal((H, W))
    eng = ap.Engine(L.PROB_TV2D, s=np.asfortranarray(img).reshape(-1, order="F"), lam=1.0, shape=(H, W))
    cases = [("anisotropic", 0)] + ([("isotropic", 1)] if hasattr(eng, "set_tv2d_isotropic") else [])
    cases = [c for c in cases if c[0] in args.cases]
    kw = dict(domaxiters=1, record_history=0, rho=args.rho)

    def select(iso):
        if hasattr(eng, "set_tv2d_isotropic"):
            eng.set_tv2d_isotropic(bool(iso))

    rows = []
    try:
        per = {name: [] for name, _ in cases}
        pix = {name: [] for name, _ in cases}
        xsol = {name: [] for name, _ in cases}
        eng.set_profiling(False)
        for name, iso in cases:  # warm-up of every kernel either form launches
            select(iso)
            assert float(eng.run(maxiters=args.short, **kw).steps) == args.short
            assert float(eng.fetch(L.F_CG_ITERS, 1)[0]) == 0.0, "not the spectral path"
        for _ in range(args.reps):
            for name, iso in cases:
                select(iso)
                t_short = eng.run(maxiters=args.short, **kw).runtime_s
                t_long = eng.run(maxiters=args.long, **kw).runtime_s
                per[name].append((t_long - t_short) / (args.long - args.short) * 1e6)
        eng.set_profiling([L.K_PROX, L.K_XSOLVE], stride=4)
        for _ in range(args.reps):
            for name, iso in cases:
                select(iso)
                eng.run(maxiters=args.long, **kw)
                for which, out in ((L.K_PROX, pix), (L.K_XSOLVE, xsol)):
                    ms, cnt = eng.kernel_time(which)
                    out[name].append(ms / max(cnt, 1) * 1e3)
        for name, _ in cases:
            med = lambda v: round(float(np.median(v)), 2)
            rows.append(dict(H=H, W=W, rho=args.rho, case=name, us_per_iter=med(per[name]),
                             us_min=round(float(np.min(per[name])), 2), us_max=round(float(np.max(per[name])), 2),
                             pixel_pass_us=med(pix[name]), pixel_pass_us_min=round(float(np.min(pix[name])), 2),
                             pixel_pass_us_max=round(float(np.max(pix[name])), 2), xsolve_us=med(xsol[name]),
                             xsolve_us_min=round(float(np.min(xsol[name])), 2),
                             xsolve_us_max=round(float(np.max(xsol[name])), 2), reps=args.reps,
                             iters=[args.short, args.long]))
            print(json.dumps(rows[-1]), flush=True)
    finally:
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
