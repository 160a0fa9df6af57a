"""Group-lasso logistic regression on one-hot data: the regularisation path of groupclassifier_path.
Twelve categorical variables of six levels each are one-hot coded behind a column of ones; the labels depend on the first
four variables alone.  Every lambda of the path runs side by side in one object over one sparse D, and the columns of a
variable enter the model together: df_groups counts variables, not columns.

    python examples/group_logistic_path.py
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import admm_project_amd as ap  # noqa: E402


def main(rows=4096, variables=12, levels=6, used=4, seed=0):
    rng = np.random.default_rng(seed)
    cat = rng.integers(0, levels, (rows, variables))
    n = 1 + variables * levels
    col = 1 + cat + levels * np.arange(variables)[None, :]
    onehot = sp.csc_matrix((np.ones(rows * variables), (np.repeat(np.arange(rows), variables), col.reshape(-1))),
                           shape=(rows, n))
    D = sp.csc_matrix(sp.hstack([sp.csc_matrix(np.ones((rows, 1))), onehot[:, 1:]]))
    truth = np.zeros(n)
    for v in range(used):
        eff = rng.choice([-1.0, 1.0], levels) * rng.uniform(1.0, 2.0, levels)
        truth[1 + v * levels:1 + (v + 1) * levels] = eff - eff.mean()
    score = D @ truth
    ell = np.where(score + 0.1 * np.std(score) * rng.standard_normal(rows) >= 0, 1.0, -1.0)
    groups = [1] + [levels] * variables
    weights = [0.0] + [np.sqrt(levels)] * variables  # the intercept is not penalised
    res = ap.groupclassifier_path(D, ell, groups, None, dict(groupweights=weights, objevals=1))
    print(f"{rows} x {n}, {D.nnz} nonzeros, {len(groups)} groups; one run of {res['runtime'] * 1e3:.1f} ms")
    print("  lambda      steps  columns  variables  training accuracy")
    for k, lam in enumerate(res["lams"]):
        z2 = res["zopt"][rows:, k]
        acc = float(np.mean(np.where(D @ z2 >= 0, 1.0, -1.0) == ell))
        print(f"  {lam:10.4g}  {int(res['steps'][k]):5d}  {int(res['df'][k]):7d}  {int(res['df_groups'][k]) - 1:9d}  {acc:.3f}")


if __name__ == "__main__":
    main()
