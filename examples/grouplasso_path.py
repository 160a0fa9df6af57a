"""A group-lasso regularisation path: ten lambda values from the group lambda_max down to a hundredth of
it, fitted side by side in ONE run -- on a dense design matrix over one cached inverse, on a sparse one over one CSR
product -- with whole groups of coefficients entering as lambda falls.

    python examples/grouplasso_path.py [rows cols group] [sparse]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402

argv = [a for a in sys.argv[1:] if a != "sparse"]
rows, cols, group = (int(argv[0]), int(argv[1]), int(argv[2])) if len(argv) >= 3 else (3000, 2000, 10)
sparse = "sparse" in sys.argv[1:]

D = (ap.synth.sparse_lasso_problem(0, rows, cols, 0.05) if sparse else ap.synth.lasso_problem(0, rows, cols))["D"]
sizes = np.full(cols // group, group, dtype=np.int64)
sizes[-1] += cols - int(sizes.sum())
rng = np.random.default_rng(1)
live = np.repeat(rng.random(sizes.size) < 0.1, sizes)  # a tenth of the groups carry signal
truth = np.where(live, rng.choice([-1.0, 1.0], cols) * rng.uniform(1.0, 3.0, cols), 0.0)
s = D @ truth + np.sqrt(0.001) * rng.standard_normal(rows)

res = ap.grouplasso_path(D, s, sizes, None, dict(objevals=1, groupweights=np.sqrt(sizes)))
print(f"{res['lams'].size} lambda values on {rows} x {cols}, {sizes.size} groups (x-update: {res['xsolve']}): steps "
      f"{res['steps'].min()}..{res['steps'].max()}, loop {res['runtime'] * 1e3:.1f} ms, setup + loop "
      f"{res['solverruntime'] * 1e3:.1f} ms")
first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
planted = np.add.reduceat(live, first) > 0
for k, lam in enumerate(res["lams"]):
    on = np.add.reduceat(res["zopt"][:, k] != 0, first) > 0
    print(f"lambda = {lam:9.4f} ({lam / res['lams'][0]:5.3f} lambda_max): {int(res['df_groups'][k]):4d} live groups, "
          f"{int(np.sum(on & planted))} of the {int(planted.sum())} planted ones, objective {res['objopt'][k]:.4f}")
