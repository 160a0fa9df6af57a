"""The lasso on a sparse design matrix, all legs in one process: 100000 x 10000 at density 1 % and 0.1 %,
the 0.1 % matrix with 100 rows of 5000 nonzeros (skew), and the dense xsolve = cg engine on the 1 % matrix densified --
the existing code, and the yardstick: the sparse inner iteration must beat it.

Per leg: microseconds per ADMM iteration and per inner CG iteration from the loop's own runtime (a forced run length,
runtime / iterations and runtime / inner iterations), the two products of one inner iteration timed with HIP events
around their launches (a run of its own), the bytes they move -- 2 * nnz * 12 B plus the row starts and the vectors;
16 * m * n B for the dense pair -- per second, and the lanes per row each orientation's plan chose.

    python profiles/sparse_lasso_bench.py [--shape 100000x10000] [--iters 20] [--reps 3] [--no-dense] [--out file.json]
prints one JSON line per leg.
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402


def skewed(D, nrows, per_row, seed):
    """D with ``nrows`` of its rows filled to ``per_row`` nonzeros, columns renormalised"""
    rng = np.random.default_rng(seed)
    m, n = D.shape
    rows = rng.choice(m, size=nrows, replace=False)
    r = np.repeat(rows, per_row)
    c = np.concatenate([rng.choice(n, size=per_row, replace=False) for _ in rows])
    S = sp.csc_matrix(D + sp.coo_matrix((rng.standard_normal(r.size), (r, c)), shape=D.shape))
    nrm = np.sqrt(np.asarray(S.multiply(S).sum(axis=0)).ravel())
    return sp.csc_matrix(S @ sp.diags(1.0 / np.where(nrm > 0.0, nrm, 1.0)))


def leg(name, D, s, lam, args, dense=False):
    L = ap._lib
    m, n = D.shape
    if dense:
        eng = ap.Engine(L.PROB_LASSO, D=np.asfortranarray(D.toarray()), s=s, lam=lam, xsolve=L.XSOLVE_CG)
    else:
        eng = ap.Engine(L.PROB_LASSO, D=D, s=s, lam=lam)
    try:
        kw = dict(domaxiters=1, record_history=0, maxiters=args.iters)
        eng.set_profiling(False)
        eng.run(**kw)  # warm-up
        per_iter, per_inner, inner = [], [], 0
        for _ in range(args.reps):
            t = eng.run(**kw).runtime_s
            cg = eng.fetch(L.F_CG_ITERS, 2)
            inner = int(cg[0])
            per_iter.append(t / args.iters * 1e6)
            per_inner.append(t / max(inner, 1) * 1e6)
        eng.set_profiling([L.K_GEMV_N, L.K_GEMV_T])
        eng.run(**kw)
        (ms_n, cnt_n), (ms_t, cnt_t) = eng.kernel_time(L.K_GEMV_N), eng.kernel_time(L.K_GEMV_T)
        us_n, us_t = ms_n / max(cnt_n, 1) * 1e3, ms_t / max(cnt_t, 1) * 1e3
        nnz = int(D.nnz)
        moved = 16.0 * m * n if dense else 2.0 * nnz * 12 + 8.0 * 2 * (m + n) + 8.0 * 2 * (m + n)
        info = eng.sparse_info() if not dense else None
        row = dict(leg=name, m=m, n=n, nnz=nnz, density=round(nnz / (m * n), 6), engine="dense cg" if dense else "sparse",
                   us_per_admm_iter=round(float(np.median(per_iter)), 1),
                   us_per_inner_iter=round(float(np.median(per_inner)), 2),
                   us_per_inner_iter_min=round(float(np.min(per_inner)), 2),
                   us_per_inner_iter_max=round(float(np.max(per_inner)), 2),
                   inner_iters=inner, admm_iters=args.iters, product_n_us=round(us_n, 2), product_t_us=round(us_t, 2),
                   bytes_per_inner_iter=int(moved), tb_per_s=round(moved / ((us_n + us_t) * 1e-6) / 1e12, 3),
                   lanes=None if dense else list(info["lanes"]), capped_updates=int(cg[1]),
                   setup_s=round(eng.setup_seconds, 3), reps=args.reps)
        print(json.dumps(row), flush=True)
        return row
    finally:
        eng.close()


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--shape", default="100000x10000")
    a.add_argument("--iters", type=int, default=20)
    a.add_argument("--reps", type=int, default=3)
    a.add_argument("--no-dense", action="store_true")
    a.add_argument("--out", default=None)
    args = a.parse_args()
    ap._lib.require_device()
    m, n = (int(v) for v in args.shape.split("x"))
    rows = []
    p1 = ap.synth.sparse_lasso_problem(0, m, n, 0.01)
    rows.append(leg("1 %", p1["D"], p1["s"], p1["lam"], args))
    p01 = ap.synth.sparse_lasso_problem(1, m, n, 0.001)
    rows.append(leg("0.1 %", p01["D"], p01["s"], p01["lam"], args))
    Dk = skewed(p01["D"], min(100, m), min(5000, n), 2)
    rows.append(leg("0.1 % + 100 rows of 5000", Dk, p01["s"], 0.1 * float(np.max(np.abs(Dk.T @ p01["s"]))), args))
    if not args.no_dense:
        rows.append(leg("1 % densified", p1["D"], p1["s"], p1["lam"], args, dense=True))
        rows[-1]["sparse_inner_is_faster"] = rows[0]["us_per_inner_iter"] < rows[-1]["us_per_inner_iter"]
        print(json.dumps(dict(sparse_inner_us=rows[0]["us_per_inner_iter"], dense_inner_us=rows[-1]["us_per_inner_iter"],
                              sparse_inner_is_faster=rows[-1]["sparse_inner_is_faster"])), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    if not args.no_dense and not rows[-1]["sparse_inner_is_faster"]:
        sys.exit("the sparse inner iteration is not faster than the dense one: the kernel is wrong, not slow")


if __name__ == "__main__":
    main()
