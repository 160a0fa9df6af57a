"""A regularisation path of the l1-regularised multinomial (softmax) logistic model on a synthetic bag-of-words matrix:
documents x terms, sparse counts scaled to unit columns, four topics.  Every lambda is one model of four classes; the
models of the path run side by side in ONE object over one upload of D, each to its own stop.

    python examples/sparse_text_multinomial_path.py [documents] [terms]
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402


def corpus(docs, terms, topics=4, seed=0):
    """term counts drawn from a topic's own term distribution over a shared background; the label is the topic"""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, topics, docs)
    base = rng.dirichlet(np.full(terms, 0.05))
    own = np.stack([rng.dirichlet(np.full(terms, 0.02)) for _ in range(topics)])
    rows, cols, vals = [], [], []
    for i in range(docs):
        counts = rng.multinomial(60, 0.7 * base + 0.3 * own[y[i]])
        j = np.flatnonzero(counts)
        rows += [i] * j.size
        cols += j.tolist()
        vals += np.log1p(counts[j]).tolist()
    D = sp.csc_matrix((vals, (rows, cols)), shape=(docs, terms))
    nrm = np.sqrt(np.asarray(D.multiply(D).sum(axis=0))).reshape(-1)
    return (D @ sp.diags(1.0 / np.where(nrm > 0, nrm, 1.0))).tocsc(), y


def main():
    docs = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
    terms = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    D, y = corpus(docs, terms)
    train = np.arange(docs) < (3 * docs) // 4
    res = ap.multinomial_path(D[train], y[train], 6, dict(objevals=1, lambda_min_ratio=0.02, maxiters=400))
    print(f"{int(train.sum())} documents x {terms} terms, nnz {res['nnz']}, classes {res['classes'].tolist()}, "
          f"loop {res['runtime'] * 1e3:.1f} ms")
    print(f"{'lambda':>10} {'steps':>6} {'df':>5} {'objective':>12} {'held-out accuracy':>18}")
    for j, lam in enumerate(res["lams"]):
        X = res["zopt"][int(train.sum()):, :, j]  # the sparse coefficient block
        proba = ap.multinomial_proba(D[~train], X)
        acc = float(np.mean(res["classes"][np.argmax(proba, axis=1)] == y[~train]))
        print(f"{lam:10.4f} {res['steps'][j]:6d} {res['df'][j]:5d} {res['objopt'][j]:12.4f} {acc:18.3f}")


if __name__ == "__main__":
    main()
