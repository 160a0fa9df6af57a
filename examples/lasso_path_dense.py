"""A lasso regularisation path on a dense design matrix: ten lambda values from lambda_max down to a
hundredth of it, fitted side by side in ONE run -- the factor of D'D + rho*I and its inverse are built once, and every
iteration reads the inverse once for all ten fits.

    python examples/lasso_path_dense.py [rows cols]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402

argv = sys.argv[1:]
rows, cols = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (3000, 2000)

p = ap.synth.lasso_path_problem(seed=0, rows=rows, cols=cols)
D, s, truth = p["D"], p["s"], p["testx"]
res = ap.lasso_path_dense(D, s, None, dict(objevals=1))
print(f"{res['lams'].size} lambda values on {rows} x {cols} (x-update: {res['xsolve']}): steps {res['steps'].min()}.."
      f"{res['steps'].max()}, loop {res['runtime'] * 1e3:.1f} ms, setup + loop {res['solverruntime'] * 1e3:.1f} ms")
support = truth != 0
for k, lam in enumerate(res["lams"]):
    z = res["zopt"][:, k]
    hit = int(np.sum((z != 0) & support))
    print(f"lambda = {lam:9.4f} ({lam / p['lmax']:5.3f} lambda_max): {int(res['df'][k]):5d} nonzeros, {hit} of the "
          f"{int(support.sum())} planted ones, objective {res['objopt'][k]:.4f}")
