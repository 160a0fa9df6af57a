"""A covariance-selection (graphical lasso) regularisation path: ten lambda values from lambda_max --
where the selected graph is empty -- down to a hundredth of it, fitted side by side in ONE run, every fit in a workgroup
of its own with the whole ADMM iteration in one kernel.

    python examples/covsel_path.py [samples variables]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402

argv = sys.argv[1:]
rows, cols = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (2000, 64)

p = ap.synth.covsel_problem(seed=0, rows=rows, cols=cols)
D, Sinv = p["D"], p["Sinv"]
truth = np.triu(Sinv != 0, k=1)
res = ap.covarianceselection_path(D, None, dict(objevals=1))
lmax = ap.covarianceselection_lambda_max(D)
print(f"{res['lams'].size} lambda values, {rows} samples of {cols} variables: steps {res['steps'].min()}.."
      f"{res['steps'].max()}, loop {res['runtime'] * 1e3:.1f} ms, setup + loop {res['solverruntime'] * 1e3:.1f} ms")
for k, lam in enumerate(res["lams"]):
    edges = np.triu(res["zopt"][:, :, k] != 0, k=1)
    print(f"lambda = {lam:8.5f} ({lam / lmax:5.3f} lambda_max): {int(res['df'][k]):5d} edges, "
          f"{int(np.sum(edges & truth))} of the {int(truth.sum())} planted ones, objective {res['objopt'][k]:.4f}")
