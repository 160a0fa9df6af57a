"""Cross-validated l1-regularised logistic regression on a sparse bag-of-words-like matrix: five folds
times ten lambda values plus the ten full-data fits -- sixty classifiers -- in ONE run over one upload of D.  A fold fit
leaves its rows out through their cost (a held-out row costs 0), so no row-subset matrix is ever built.

    python examples/sparse_text_logistic_cv.py [documents words density]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402

argv = sys.argv[1:]
rows, cols = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (20000, 2000)
density = float(argv[2]) if len(argv) >= 3 else 0.01

p = ap.synth.sparse_design_classifier_problem(seed=0, rows=rows, cols=cols, density=density)
D, ell, truth = p["D"], p["ell"], p["testx"]
res = ap.l1classifier_cv(D, ell, None, dict(nfolds=5, seed=0, nodualerror=1))
F, L = res["heldout_loss"].shape
print(f"{F} folds x {L} lambda values + {L} full-data fits on {rows} x {cols}, {res['nnz']} nonzeros: loop "
      f"{res['runtime'] * 1e3:.1f} ms, setup + loop {res['solverruntime'] * 1e3:.1f} ms, "
      f"{int(res['cg_iters_total'].sum())} inner CG iterations over all fits")
support = truth != 0
rate = res["heldout_errors"].sum(axis=0) / res["heldout_weight"].sum(axis=0)
for k, lam in enumerate(res["lams"]):
    z = res["zopt"][rows:, k]
    mark = " <- lam_min" if k == res["index_min"] else (" <- lam_1se" if k == res["index_1se"] else "")
    print(f"lambda = {lam:9.4f}: held-out deviance {res['cvm'][k]:.5f} +- {res['cvsd'][k]:.5f}, error rate {rate[k]:.4f}, "
          f"{int(res['df'][k]):5d} nonzeros, {int(np.sum((z != 0) & support))} of the {int(support.sum())} planted "
          f"ones{mark}")
