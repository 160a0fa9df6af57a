"""An l1-regularised logistic regression path on a dense design matrix: ten lambda values from
lambda_max down to a hundredth of it, fitted side by side in ONE run -- the inverse of D'D + I is built once, and every
iteration reads D twice for all ten fits.

    python examples/sparse_logistic_path.py [rows cols]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402

argv = sys.argv[1:]
rows, cols = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (3000, 2000)

p = ap.synth.sparse_classifier_problem(seed=0, rows=rows, cols=cols)
D, ell, truth = p["D"], p["ell"], p["testx"]
res = ap.l1classifier_path(D, ell, 10, dict(objevals=1, lossfunction="logistic"))
print(f"{res['lams'].size} lambda values on {rows} x {cols} (x-update: {res['xsolve']}): steps {res['steps'].min()}.."
      f"{res['steps'].max()}, loop {res['runtime'] * 1e3:.1f} ms, setup + loop {res['solverruntime'] * 1e3:.1f} ms")
support = truth != 0
for k, lam in enumerate(res["lams"]):
    z = res["zopt"][rows:, k]
    hit = int(np.sum((z != 0) & support))
    acc = float(np.mean(np.where(D @ z >= 0, 1.0, -1.0) == ell))
    print(f"lambda = {lam:9.4f} ({lam / res['lams'][0]:5.3f} lambda_max): {int(res['df'][k]):5d} nonzeros, {hit} of the "
          f"{int(support.sum())} planted ones, training accuracy {acc:.3f}, objective {res['objopt'][k]:.4f}")
