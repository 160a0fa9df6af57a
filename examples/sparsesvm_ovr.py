"""A multi-class linear SVM on a sparse design matrix: one-vs-rest classifiers for every class of a
text-like matrix, trained in ONE run -- the matrix stays sparse on the device (24 B per nonzero), the x-update is
conjugate gradients for all classes in lock-step over one sparse product, and nothing n x n is built.

    python examples/sparsesvm_ovr.py [rows cols density classes]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402

argv = sys.argv[1:]
rows, cols = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (20000, 2000)
density = float(argv[2]) if len(argv) >= 3 else 0.01
K = int(argv[3]) if len(argv) >= 4 else 5

p = ap.synth.sparse_svm_problem(seed=0, rows=rows, cols=cols, density=density, classes=K)
D, labels = p["D"], p["labels"]
res = ap.linearsvm_ovr(D, labels, p["C"], dict(classes=np.arange(float(K)), lossfunction="hinge", objevals=1))
print(f"{K} classifiers on {rows} x {cols}, {res['nnz']} nonzeros ({D.nnz * 24 / 2 ** 20:.1f} MiB on the device, "
      f"{rows * cols * 8 / 2 ** 20:.0f} MiB dense): steps {res['steps'].min()}..{res['steps'].max()}, "
      f"loop {res['runtime'] * 1e3:.1f} ms, setup + loop {res['solverruntime'] * 1e3:.1f} ms")
print(f"inner CG iterations per class {list(res['cg_iters_total'])}, x-updates that ended on cg_maxit "
      f"{list(res['cg_capped_updates'])}")
pred = np.argmax(D @ res["xopt"], axis=1)
print(f"training accuracy of argmax_c (D*x_c): {np.mean(pred == labels) * 100:.2f} %")
