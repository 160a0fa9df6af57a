"""A lasso regularisation path on a sparse design matrix: ten lambda values from lambda_max down to a
hundredth of it, fitted side by side in ONE run -- the matrix stays sparse on the device (24 B per nonzero), every
x-update is conjugate gradients on (D'D + rho*I) x = D's + rho*(z - u) for all lambda in lock-step over one sparse
product, and nothing n x n is built.

    python examples/sparse_lasso_path.py [rows cols density]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402

argv = sys.argv[1:]
rows, cols = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (20000, 2000)
density = float(argv[2]) if len(argv) >= 3 else 0.01

p = ap.synth.sparse_lasso_path_problem(seed=0, rows=rows, cols=cols, density=density)
D, s, truth = p["D"], p["s"], p["testx"]
res = ap.lasso_path(D, s, None, dict(objevals=1))
print(f"{res['lams'].size} lambda values on {rows} x {cols}, {res['nnz']} nonzeros ({D.nnz * 24 / 2 ** 20:.1f} MiB on the "
      f"device): steps {res['steps'].min()}..{res['steps'].max()}, loop {res['runtime'] * 1e3:.1f} ms, "
      f"setup + loop {res['solverruntime'] * 1e3:.1f} ms")
print(f"inner CG iterations per fit {res['cg_iters_total'].tolist()}, x-updates that ended on cg_maxit "
      f"{res['cg_capped_updates'].tolist()}")
support = truth != 0
for k, lam in enumerate(res["lams"]):
    z = res["zopt"][:, k]
    hit = int(np.sum((z != 0) & support))
    print(f"lambda = {lam:9.4f} ({lam / p['lmax']:5.3f} lambda_max): {int(res['df'][k]):5d} nonzeros, {hit} of the "
          f"{int(support.sum())} planted ones, objective {res['objopt'][k]:.4f}")
