"""Inputs and CPU references of the multi-fit regression tests (a helper of test_gpu_reg_multi / test_reg_multi_host, not
a test): the seven fits, the shapes at the pass kernel's edges, and per fit the oracle's loop with the
restated prox (tests/loss_restated.py) under nodualerror = 1 -- computed once per case and shared."""
import functools

import numpy as np

import loss_restated as R

# the K = 7 fits of one run: LAD, two quantiles, the epsilon-insensitive loss, Huber at delta = 1, an asymmetric Huber
# at delta = 0.25, and a second LAD fit (under the shared weights of the weighted cases: a LAD fit with zero weights)
FITS = (
    dict(kind="lad"),
    dict(kind="lad", tau=0.1),
    dict(kind="lad", tau=0.9),
    dict(kind="lad", epsilon=0.3),
    dict(kind="huber", delta=1.0),
    dict(kind="huber", delta=0.25, slopes=(2.0, 0.5)),
    dict(kind="lad"),
)
# (m, n): one block; one row in a second block; one column into a wave's second column slot (8 waves x 7 = 56 < 57);
# the limit n = 448; more 64-row blocks (258) than workgroups (256), so a workgroup takes several blocks
SHAPES = ((64, 1), (65, 8), (200, 57), (1000, 448), (16450, 24))
MODES = ("shared", "perfit", "weighted")  # one s for all fits | one column of S per fit | shared s and shared weights
MAXITERS = 40


def loss_of(fit, weights=None):
    kind = "lad" if fit["kind"] == "lad" else "huberfit"
    slopes = (fit["tau"], 1.0 - fit["tau"]) if "tau" in fit else fit.get("slopes", (1.0, 1.0))
    return R.Loss(kind, weights=weights, slopes=slopes, epsilon=fit.get("epsilon", 0.0), delta=fit.get("delta", 1.0))


def problem(m, n, seed):
    """an intercept column and n - 1 standard normal ones, heteroscedastic noise (synth.quantile_problem's recipe, which
    needs n >= 2, extended to n = 1)"""
    rng = np.random.default_rng(seed)
    D = np.asfortranarray(np.column_stack([np.ones(m), rng.standard_normal((m, n - 1))]))
    xtrue = rng.standard_normal(n)
    g = D[:, 1] if n > 1 else rng.standard_normal(m)
    s = D @ xtrue + (1.0 + 0.5 * np.abs(g)) * rng.standard_normal(m)
    return D, s


SEEDS = {(64, 1): 3, (65, 8): 4, (200, 57): 5, (1000, 448): 6, (16450, 24): 7}


@functools.lru_cache(maxsize=None)
def case(shape, mode):
    """(D, S, weights) of one case: S is m x 1 (shared, weighted) or m x 7 (perfit: s scaled and shifted per fit)"""
    m, n = shape
    D, s = problem(m, n, SEEDS[shape])
    rng = np.random.default_rng(SEEDS[shape] + 100)
    if mode == "perfit":
        S = np.asfortranarray(np.column_stack([(1.0 + 0.15 * k) * s + 0.2 * k + 0.3 * rng.standard_normal(m)
                                               for k in range(len(FITS))]))
    else:
        S = np.asfortranarray(s.reshape(-1, 1))
    w = None
    if mode == "weighted":
        w = rng.uniform(0.5, 2.0, m)
        w[::7] = 0.0  # observations that do not count
    return D, S, w


@functools.lru_cache(maxsize=None)
def reference(shape, mode):
    """per fit: loss_restated.run(kind, D, s_k, Loss(...), nodualerror = 1, objevals = 1, maxiters = MAXITERS)"""
    D, S, w = case(shape, mode)
    out = []
    for k, fit in enumerate(FITS):
        loss = loss_of(fit, w)
        s = S[:, k if S.shape[1] > 1 else 0]
        out.append(R.run(loss.kind, D, np.ascontiguousarray(s), loss, dict(nodualerror=1, objevals=1, maxiters=MAXITERS)))
    return out


def knife_edge(ref):
    """the smallest |pnorm - perr| / perr over the last two iterations of every fit"""
    worst = np.inf
    for r in ref:
        pn, pe = np.asarray(r["pnorm"]), np.asarray(r["perr"])
        for i in range(max(0, len(pn) - 2), len(pn)):
            worst = min(worst, abs(pn[i] - pe[i]) / pe[i])
    return worst
