"""Several quantiles of one response on a sparse design matrix: K quantile regressions over a one-hot /
text-like matrix with a dense intercept column, fitted in ONE run -- the matrix stays sparse on the device (24 B per
nonzero), the x-update is conjugate gradients for all quantiles in lock-step over one sparse product, and nothing n x n
is built.

    python examples/sparse_quantiles.py [rows cols density]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402

argv = sys.argv[1:]
rows, cols = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (20000, 2000)
density = float(argv[2]) if len(argv) >= 3 else 0.01
taus = (0.05, 0.25, 0.5, 0.75, 0.95)

p = ap.synth.sparse_regression_problem(seed=0, rows=rows, cols=cols, density=density)
D, s = p["D"], p["s"]
res = ap.quantilereg_multi(D, s, taus, dict(objevals=1))
print(f"{len(taus)} quantiles on {rows} x {cols}, {res['nnz']} nonzeros ({D.nnz * 24 / 2 ** 20:.1f} MiB on the device, "
      f"{rows * cols * 8 / 2 ** 20:.0f} MiB dense): steps {res['steps'].min()}..{res['steps'].max()}, "
      f"loop {res['runtime'] * 1e3:.1f} ms, setup + loop {res['solverruntime'] * 1e3:.1f} ms")
print(f"inner CG iterations per fit {res['cg_iters_total'].tolist()}, x-updates that ended on cg_maxit "
      f"{res['cg_capped_updates'].tolist()}")
Z = res["zopt"]  # the residuals D*x - s of every fit
for k, tau in enumerate(taus):
    print(f"tau = {tau:4.2f}: {np.mean(Z[:, k] < 0) * 100:6.2f} % of the residuals below zero, "
          f"{int(np.sum(Z[:, k] == 0))} exactly on the fit, pinball loss {res['objopt'][k]:.4f}")
