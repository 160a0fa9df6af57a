"""An l1-regularised logistic regression path on a bag-of-words-like SPARSE matrix: documents x terms with
Zipf-distributed term frequencies, tf-idf-like positive entries, unit columns; two classes that differ in a few dozen
planted terms.  Ten lambda values from lambda_max down to a hundredth of it are fitted side by side in ONE run: every
x-update is conjugate gradients on (D'D + I) over one sparse product for all ten fits, and nothing terms x terms is stored.

    python examples/sparse_text_logistic_path.py [documents terms words_per_document]
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402

argv = sys.argv[1:]
docs, terms, words = (int(argv[0]), int(argv[1]), int(argv[2])) if len(argv) >= 3 else (20000, 5000, 40)

rng = np.random.default_rng(0)
freq = 1.0 / np.arange(1, terms + 1) ** 0.9  # Zipf: a few terms in most documents, most terms in a few
freq /= freq.sum()
planted = rng.choice(np.arange(20, terms // 2), 30, replace=False)  # neither the stop words nor the rarest terms
truth = np.zeros(terms)
truth[planted] = rng.choice([-1.0, 1.0], planted.size) * rng.uniform(1.0, 3.0, planted.size)
rows = np.repeat(np.arange(docs), words)
cols = rng.choice(terms, size=docs * words, p=freq)
counts = sp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(docs, terms)).tocsc()  # (duplicates add up: counts)
counts.data = 1.0 + np.log(counts.data)  # damped term frequency
nrm = np.sqrt(np.asarray(counts.multiply(counts).sum(axis=0))).reshape(-1)
D = (counts @ sp.diags(1.0 / np.where(nrm > 0, nrm, 1.0))).tocsc()
score = D @ truth
ell = np.where(score + 0.1 * float(np.std(score)) * rng.standard_normal(docs) >= 0, 1.0, -1.0)

res = ap.l1classifier_path(D, ell, 10, dict(objevals=1, lossfunction="logistic"))
print(f"{res['lams'].size} lambda values on {docs} x {terms}, {D.nnz} nonzeros ({100.0 * D.nnz / (docs * terms):.2f} %), "
      f"x-update: {res['xsolve']}: steps {res['steps'].min()}..{res['steps'].max()}, inner iterations "
      f"{res['cg_iters_total'].min()}..{res['cg_iters_total'].max()}, loop {res['runtime'] * 1e3:.1f} ms, setup + loop "
      f"{res['solverruntime'] * 1e3:.1f} ms")
support = truth != 0
for k, lam in enumerate(res["lams"]):
    z = res["zopt"][docs:, k]
    hit = int(np.sum((z != 0) & support))
    acc = float(np.mean(np.where(D @ z >= 0, 1.0, -1.0) == ell))
    print(f"lambda = {lam:9.4f} ({lam / res['lams'][0]:5.3f} lambda_max): {int(res['df'][k]):5d} nonzeros, {hit} of the "
          f"{int(support.sum())} planted ones, training accuracy {acc:.3f}, objective {res['objopt'][k]:.4f}")
