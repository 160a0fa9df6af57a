"""The multinomial (softmax) model on the host: the restated run (multinomial_restated) satisfies the
optimality conditions, lambda_max is the threshold of the all-zero model, the slot map round-trips, the Python functions
refuse bad arguments before any device work, and the two figures the device tests take their bounds from -- PROX_RATIO
and MEASURED_GAP -- are measured here and held against their records.

The plan of q49 named one more check -- Cn = 2 against a restated binary logistic fit at 2 lambda, 2 mu -- on the
condition that the equivalence holds for the PENALISED problem.  It does not hold iterate by iterate: the two-class loss
depends on x_0 - x_1 alone, so under the pure l1 penalty every split of b = x_0 - x_1 between the classes with one sign
has the same objective lambda*|b| (the minimiser is not unique), and the ADMM iterates of the two problems differ.  The
check is left out."""
import numpy as np
import pytest

import multinomial_restated as R
from admm_project_amd import softmax as M

SHAPE = (120, 30)


def _problem(Cn, seed=0):
    rng = np.random.default_rng(100 * Cn + seed)
    D = rng.standard_normal(SHAPE)
    D /= np.linalg.norm(D, axis=0)
    W = np.where(rng.random((SHAPE[1], Cn)) < 0.2, 3.0 * rng.standard_normal((SHAPE[1], Cn)), 0.0)
    y = np.argmax(D @ W + 0.05 * rng.standard_normal((SHAPE[0], Cn)), axis=1).astype(np.int64)
    y[:Cn] = np.arange(Cn)
    return D, y


# ------------------------------------------------------------------------------------------------------------- 1. KKT
@pytest.mark.parametrize("Cn", (3, 5))
def test_the_restated_run_satisfies_the_optimality_conditions(Cn):
    """test_l1class_host's argument on the stacked problem: at the stop, D'grad L(z1) + q = delta per class with q in the
    penalty's subdifferential at z2 and ||delta|| < derr; kkt is evaluated at X := z2, where the loss's gradient is taken
    at D*z2 instead of z1, and z1 - D*z2 is bounded by (1 + ||D||)*perr.  The softmax gradient is Lipschitz with constant
    C*max(c)*1/2 (the Hessian diag p - p p' has norm <= 1/2).  Hence
        violation <= derr + ||D||_2 * Lphi * (1 + ||D||_2) * perr."""
    D, y = _problem(Cn)
    mo = R.Model(ridge=0.05)
    mo.lam = 0.3 * R.lambda_max(D, y, mo, Cn)
    res = R.run_cholesky(D, y, Cn, mo, dict(abstol=1e-10, reltol=1e-10, maxiters=200000))
    assert res["steps"] < 200000
    Z2 = res["zopt"][SHAPE[0]:]
    nD = np.linalg.norm(D, 2)
    bound = res["derr"][-1] + nD * (mo.C * 0.5) * (1.0 + nD) * res["perr"][-1]
    viol = R.kkt(D, y, mo, Z2)
    print(f"Cn {Cn}: steps {res['steps']}, kkt violation {viol:.3e}, bound {bound:.3e}, nonzeros {np.count_nonzero(Z2)}")
    assert 0 < np.count_nonzero(Z2) < Z2.size
    assert viol <= bound
    assert R.kkt(D, y, mo, np.zeros_like(Z2)) > 0.1 * mo.lam  # and kkt notices a wrong point


# ------------------------------------------------------------------------------------------------------ 2. lambda_max
def test_lambda_max_is_the_threshold_of_the_zero_model():
    D, y = _problem(4)
    w = np.linspace(0.5, 2.0, SHAPE[1])
    o = dict(weights=np.linspace(0.5, 1.5, SHAPE[0]), classweight="balanced", l1weights=w, C=2.0)
    mo = R.Model(l1weights=w, weights=o["weights"], classweight="balanced", C=2.0)
    lmax = M.multinomial_lambda_max(D, y, o)
    assert abs(lmax - R.lambda_max(D, y, mo, 4)) <= 1e-13 * lmax
    zero = np.zeros((SHAPE[1], 4))
    mo.lam = lmax
    assert R.kkt(D, y, mo, zero) <= 1e-12 * lmax
    mo.lam = 0.9 * lmax
    assert R.kkt(D, y, mo, zero) >= 0.999 * 0.1 * lmax * w.min()  # the critical coordinate: |g_j| = lmax*w_j against 0.9*lmax*w_j
    # labels of any values: the classes are the sorted unique ones
    names = np.array(["d", "a", "c", "b"])[y]
    assert M.multinomial_lambda_max(D, names, dict(o, classweight=None)) == M.multinomial_lambda_max(
        D, np.array([3, 0, 2, 1])[y], dict(o, classweight=None))


# -------------------------------------------------------------------------------------------------------- 3. the slots
@pytest.mark.parametrize("Cn", range(2, 11))
def test_the_slot_map_round_trips(Cn):
    per = 10 // Cn
    for models in (1, per, per + 1, 3 * per + 1):
        first, K = M.slot_map(models, Cn)
        assert np.array_equal(first, R.slot_map(models, Cn)[0]) and K == R.slot_map(models, Cn)[1]
        seen = {}
        for k in range(K):
            mc = M.model_of_slot(k, Cn)
            if mc is None:
                assert k % 10 >= per * Cn
                continue
            assert first[mc[0]] + mc[1] == k
            seen.setdefault(mc[0], []).append(mc[1])
        assert sorted(seen) == list(range(models)) and all(v == list(range(Cn)) for v in seen.values())
        assert K % 10 == 0 and per * Cn == 10 or (K % 10) % Cn == 0 and K % 10 <= per * Cn  # the setter's rule
    with pytest.raises(ValueError, match="2 .. 10 classes"):
        M.slot_map(1, 11)


# ------------------------------------------------------------------------------------------------------- 4. refusals
def test_every_refusal_names_its_option():
    D, y = _problem(3)
    cases = [(dict(foldid=np.zeros(SHAPE[0])), "options.foldid is not available in multinomial"),
             (dict(heldout=[0]), "options.heldout is not available"),
             (dict(obsweights=np.ones(SHAPE[0])), "options.obsweights is not available"),
             (dict(groups=[SHAPE[1]]), "options.groups is not available"),
             (dict(comm=object()), "options.comm is not available"),
             (dict(xsolve="inverse"), "options.xsolve = 'inverse'"),
             (dict(xsolve="trsv"), "options.xsolve = 'trsv'"),
             (dict(fast=1), "options.fast is not available"),
             (dict(relax=1.5), "options.relax is not available"),
             (dict(convtest=1), "options.convtest is not available"),
             (dict(adaptive=1), "options.adaptive is not available"),
             (dict(parallel="rows"), "options.parallel is not available"),
             (dict(stopcond="hnorm"), "options.stopcond"),
             (dict(classweight=[1.0, 2.0]), "options.classweight is not 3 finite values"),
             (dict(classweight="heavy"), "options.classweight = 'heavy'"),
             (dict(weights=np.ones(3)), "weights has 3 entries"),
             (dict(l1weights=-np.ones(SHAPE[1])), "l1weights: every weight"),
             (dict(ridge=-1.0), "ridge must be"),
             (dict(nonnegative=2), "nonnegative must be 0 or 1"),
             (dict(C=0.0), "options.C"),
             (dict(z0=np.zeros(5)), "z0 is not a 150 x 3 matrix")]
    for o, match in cases:
        with pytest.raises(ValueError, match=match):
            M.multinomial(D, y, 0.1, o)
    with pytest.raises(ValueError, match="options.foldid is not available in multinomial_path"):
        M.multinomial_path(D, y, [0.1], dict(foldid=np.zeros(SHAPE[0])))
    for labels, count in ((np.zeros(SHAPE[0]), 1), (np.arange(SHAPE[0]) % 11, 11)):
        with pytest.raises(ValueError, match=f"y holds {count} distinct classes"):
            M.multinomial(D, labels, 0.1)
    with pytest.raises(ValueError, match="do not match size of y"):
        M.multinomial(D, y[:-1], 0.1)
    with pytest.raises(ValueError, match="Argument lam"):
        M.multinomial(D, y, [0.1, 0.2])
    with pytest.raises(ValueError, match="model 1: lambda"):
        M.multinomial_path(D, y, [0.1, -1.0])
    with pytest.raises(TypeError, match="not a struct"):
        M.multinomial(D, y, 0.1, 3)


# ----------------------------------------------------------------------------------------------------- 5. PROX_RATIO
def test_prox_ratio_and_the_cap():
    """the fp64 NumPy iteration on the operator test's inputs: its residual in long double in units of
    eps*max(1, ||v||_inf, a), its Newton steps against the cap, and a = 0 in bits"""
    worst, steps = 0.0, 0
    for Cn in R.PROX_CLASSES:
        for m in R.PROX_ROWS:
            V, y, a = R.prox_inputs(Cn, m)
            assert {0.0, 1e-8, 1.0, 1e6} <= set(a.tolist()) and np.abs(V).max() > 600
            assert (V.max(axis=1) == V.min(axis=1)).any() and (y == 0).any() and (y == Cn - 1).any()
            Z, iters = R.prox(V, y, a)
            assert np.array_equal(Z[a == 0], V[a == 0]) and np.all(iters[a == 0] == 0)
            ratio = float(R.residual_ratio(Z, V, y, a).max())
            print(f"Cn {Cn} m {m}: ratio {ratio:.3f}, Newton steps max {iters.max()}")
            worst, steps = max(worst, ratio), max(steps, int(iters.max()))
    print(f"PROX_RATIO measured {worst:.4f} (recorded {R.PROX_RATIO}), most Newton steps {steps} (cap {R.CAP})")
    assert steps < R.CAP
    assert worst <= R.PROX_RATIO <= 1.05 * worst + 1.0  # the record is the measured figure, rounded up


def test_a_full_newton_step_can_increase_the_merit():
    """why the iteration is damped: from z = v with a = 1e6 and the true class 700 behind, the full step lands about a
    away and ||F|| does not fall"""
    v = np.array([[-700.0, 0.0, 0.0]])
    y, a = np.array([0]), np.array([1e6])
    F, p, n2, _ = R.residual(v.copy(), v, y, a)
    g = 1.0 + a[:, None] * p
    w, q = F / g, p / g
    d = -(w + q * ((a * (p * w).sum(axis=1)) / q.sum(axis=1))[:, None])
    assert R.residual(v + d, v, y, a)[2][0] > 0.99 * n2[0]
    Z, iters = R.prox(v, y, a)
    assert 10 < iters[0] < R.CAP and R.residual_ratio(Z, v, y, a)[0] <= R.PROX_RATIO


# --------------------------------------------------------------------------------------------------- 6. MEASURED_GAP
def test_measured_gap(ap):
    """the largest relgap between the CG and the Cholesky restatement over every run test_gpu_multinomial compares with
    the CG one: per iteration (SHAPES x PARITY_CLASSES x their models x nodualerror 0 | 1), the family fit, the run at
    rho = 2.5, the tall run's shape is covered by its own Cholesky run, and the free-running runs (their gaps are in the
    records)"""
    worst, where = 0.0, None

    def take(gap, what):
        nonlocal worst, where
        if gap > worst:
            worst, where = gap, what

    for shape in R.SHAPES:
        for Cn in R.PARITY_CLASSES:
            for f in sorted(set(R.PARITY_FRACTIONS[Cn])):
                for nd in (0, 1):
                    take(R.relgap(R.parity_run(ap, shape, Cn, f, nd), R.parity_run(ap, shape, Cn, f, nd, "chol")),
                         (shape, Cn, f, nd))
        for r in R.recorded_free(shape):
            take(r["gap"], (shape, "free"))
    for nd in (0, 1):
        take(R.relgap(R.family_run(ap, R.SHAPES[0], 3, nd), R.family_run(ap, R.SHAPES[0], 3, nd, "chol")), ("family", nd))
    for f in (0.1, 0.3):
        take(R.relgap(R.parity_run(ap, R.SHAPES[0], 3, f, 0, rho=2.5), R.parity_run(ap, R.SHAPES[0], 3, f, 0, "chol", rho=2.5)),
             ("rho 2.5", f))
    c = R.case(ap, R.TALL, 3)
    mo = R.plain_model(c, 3)
    o = R.parity_options(c, 0, R.TALL_LOOP)
    take(R.relgap(R.run(c["D"], c["y"], 3, mo, o), R.run_cholesky(c["A"], c["y"], 3, mo, o)), "tall")
    print(f"MEASURED_GAP measured {worst:.3e} at {where} (recorded {R.MEASURED_GAP:.3e})")
    assert worst <= R.MEASURED_GAP <= 1.1 * worst
    assert 10.0 * R.MEASURED_GAP <= 1e-6


# ------------------------------------------------------------------------------------------------------ 7. the records
@pytest.mark.parametrize("shape", R.SHAPES)
def test_the_recorded_free_runs(ap, shape):
    """the cheapest run of every file recomputed against the record; the reference runs stop at >= FREE_DISTINCT
    distinct step counts"""
    refs = R.recorded_free(shape)
    assert len({r["steps"] for r in refs}) >= R.FREE_DISTINCT
    k = int(np.argmin([r["steps"] for r in refs]))
    again = R.free_run(ap, shape, k)
    assert again["steps"] == refs[k]["steps"]
    for key in R.RECORDED:
        assert np.array_equal(np.asarray(again[key]), np.asarray(refs[k][key])), key
