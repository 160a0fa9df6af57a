"""The multinomial (softmax) model on the sparse l1 classifier on the GPU, against the NumPy restatement
(multinomial_restated) under 10x the measured gap between its CG and Cholesky forms."""
import ctypes as C

import numpy as np
import pytest

import multinomial_restated as R
from admm_project_amd.softmax import slot_map

pytestmark = pytest.mark.gpu

BOUND = R.PARITY_BOUND
SMALL = R.SHAPES[0]
FIELDS = ("xopt", "zopt", "uopt", "pnorm", "perr", "dnorm", "derr", "objevals")


def _check(got, ref, dual, what):
    assert got["steps"] == ref["steps"], (what, got["steps"], ref["steps"])
    if not dual:
        assert "dnorm" not in got and "derr" not in got
    gap = R.relgap(got, ref)
    print(f"{what}: steps {got['steps']}, relgap {gap:.3e} (bound {BOUND:.1e})")
    assert gap <= BOUND, (what, gap)


def _bits(a, b, what):
    for key in FIELDS + ("steps", "objopt"):
        if key in a or key in b:
            x, y = np.asarray(a[key]), np.asarray(b[key])
            assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (what, key)


@pytest.mark.parametrize("nodualerror", (0, 1))
@pytest.mark.parametrize("Cn", R.PARITY_CLASSES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_every_iteration_matches_the_restated_run(gpu, shape, Cn, nodualerror):
    c = R.case(gpu, shape, Cn)
    fr = R.PARITY_FRACTIONS[Cn]
    lmax = R.lambda_max(c["A"], c["y"], R.Model(), Cn)
    assert abs(gpu.multinomial_lambda_max(c["D"], c["y"]) - lmax) <= 1e-12 * lmax
    got = gpu.multinomial_path(c["D"], c["y"], [f * lmax for f in fr],
                               dict(R.parity_options(c, nodualerror), cg_tol=R.CG_TOL))
    assert got["xopt"].shape == (shape[1], Cn, len(fr)) and got["xsolve"] == "cg"
    for j, f in enumerate(fr):
        _check(R.model_of_path(got, j), R.parity_run(gpu, shape, Cn, f, nodualerror), not nodualerror,
               f"{shape} Cn {Cn} model {j}")
    if Cn == 3:  # the copy of model 0 in the second chunk
        _bits(R.model_of_path(got, 0), R.model_of_path(got, 3), "a model in another slot of another chunk")


@pytest.mark.parametrize("shape", R.SHAPES)
def test_free_running_models_stop_where_the_restated_runs_stop(gpu, shape):
    refs = R.recorded_free(shape)
    assert len({r["steps"] for r in refs}) >= R.FREE_DISTINCT, [r["steps"] for r in refs]
    c, models = R.free_models(gpu, shape)
    got = gpu.multinomial_path(c["D"], c["y"], [mo.lam for mo in models], dict(objevals=1, cg_tol=R.CG_TOL))
    for j, ref in enumerate(refs):
        _check(R.model_of_path(got, j), ref, True, f"{shape} free model {j}")
    assert got["df"][-1] == 0 and got["df"][0] > 0  # 1.25*lambda_max: the all-zero model
    assert np.all(got["cg_capped_updates"] == 0)


@pytest.mark.parametrize("nodualerror", (0, 1))
def test_the_family_fit(gpu, nodualerror):
    """observation weights, 'balanced' class weights, a ones column with l1 weight 0, a ridge, the sign constraint"""
    c = R.family_case(gpu, SMALL, 3)
    o = dict(R.parity_options(c, nodualerror), cg_tol=R.CG_TOL, **c["model"].options())
    got = gpu.multinomial(c["D"], c["y"], c["model"].lam, o)
    _check(got, R.family_run(gpu, SMALL, 3, nodualerror), not nodualerror, "family")
    assert np.all(got["zopt"][SMALL[0]:] >= 0.0)
    # a dense ndarray runs the same object
    dense = gpu.multinomial(c["A"], c["y"], c["model"].lam, o)
    assert dense["xsolve"] == "cg"
    _bits(got, dense, "dense D through csr_matrix")


def test_five_models_over_two_chunks_and_models_alone_give_the_same_bits(gpu):
    """free-running from the zero start, 200 iterations at the most: the models at 0.6 and 1.25 of lambda_max stop on
    their own (144 and 54 steps in the restatement), the one at 0.2 runs out of iterations"""
    c = R.case(gpu, SMALL, 3)
    lmax = R.lambda_max(c["A"], c["y"], R.Model(), 3)
    lams = [f * lmax for f in (0.6, 1.25, 0.2, 1.25, 0.6)]
    o = dict(maxiters=200, objevals=1, cg_tol=R.CG_TOL)
    got = gpu.multinomial_path(c["D"], c["y"], lams, o)
    assert len(set(got["steps"].tolist())) == 3, got["steps"]  # every model stops, and freezes, as a whole and on its own
    for j, lam in enumerate(lams):
        one = gpu.multinomial(c["D"], c["y"], lam, o)
        _bits(R.model_of_path(got, j), one, f"model {j} alone")
    _bits(R.model_of_path(got, 0), R.model_of_path(got, 4), "the same model in slot 0 of chunk 0 and slot 3 of chunk 1")
    _bits(R.model_of_path(got, 1), R.model_of_path(got, 3), "the same model in slot 3 of chunk 0 and slot 0 of chunk 1")


def _object(gpu, c, Cn, lams):
    """a SparseL1Classifier that holds len(lams) plain models of case c"""
    m = c["A"].shape[0]
    first, K = slot_map(len(lams), Cn)
    ELL = np.full((m, K), -1.0, order="F")
    lk = np.zeros(K)
    for j, lam in enumerate(lams):
        for k in range(Cn):
            ELL[:, first[j] + k] = np.where(c["y"] == k, 1.0, -1.0)
            lk[first[j] + k] = lam
    return gpu.SparseL1Classifier(c["D"], ELL, lk), first, K


def _starts(c, first, K, Cn):
    out = []
    for src in (c["z0"], c["u0"]):
        full = np.zeros((src.shape[0], K), order="F")
        for f in first:
            full[:, f:f + Cn] = src
        out.append(full)
    return out


def test_two_runs_of_one_object_with_different_rho(gpu):
    c = R.case(gpu, SMALL, 3)
    lmax = R.lambda_max(c["A"], c["y"], R.Model(), 3)
    fr = (0.1, 0.3, 0.1, 0.3)  # a full chunk (slot 9 idle) and one model in a second chunk
    obj, first, K = _object(gpu, c, 3, [f * lmax for f in fr])
    assert K == 13
    try:
        obj.set_multinomial(3)
        z0, u0 = _starts(c, first, K, 3)
        for rho in (1.5, 2.5):
            res = obj.results(obj.run(rho=rho, maxiters=12, domaxiters=1, objevals=1, cg_tol=R.CG_TOL, z0=z0, u0=u0))
            for j, f in enumerate(fr):
                k0 = int(first[j])
                got = {key: res[key][:, k0:k0 + 3] for key in ("xopt", "zopt", "uopt")}
                got.update({key: res[key][:12, k0] for key in ("pnorm", "perr", "dnorm", "derr", "objevals")})
                got.update(steps=int(res["steps"][k0]), objopt=float(res["objopt"][k0]))
                _check(got, R.parity_run(gpu, SMALL, 3, f, 0, rho=rho), True, f"rho {rho} model {j}")
            assert res["steps"][9] == 0 and np.isnan(res["pnorm"][:, 9]).all()  # the idle slot never ran
    finally:
        obj.close()


def test_a_workgroup_takes_several_row_blocks(gpu):
    """8200 rows: more than 256 x 32, so a workgroup of the row kernel takes several row blocks; objevals: the loss slot"""
    c = R.case(gpu, R.TALL, 3)
    mo = R.plain_model(c, 3)
    o = R.parity_options(c, 0, R.TALL_LOOP)
    got = gpu.multinomial(c["D"], c["y"], mo.lam, dict(o, cg_tol=R.CG_TOL))
    ref = R.reference(("tall",), lambda: R.run(c["D"], c["y"], 3, mo, o))
    _check(got, ref, True, "tall")


def test_the_setter(gpu):
    L = gpu._lib
    c = R.case(gpu, SMALL, 3)
    lmax = R.lambda_max(c["A"], c["y"], R.Model(), 3)
    loop = dict(maxiters=15, domaxiters=1, objevals=1, rho=1.5)
    obj, first, K = _object(gpu, c, 3, [0.1 * lmax, 0.3 * lmax])
    fresh, _, _ = _object(gpu, c, 3, [0.1 * lmax, 0.3 * lmax])
    try:
        obj.set_multinomial(3)
        multi = obj.results(obj.run(**loop))
        obj.set_multinomial(0)  # the per-fit object again: K one-vs-rest logistic fits
        back = obj.results(obj.run(**loop))
        ovr = fresh.results(fresh.run(**loop))
        _bits(back, ovr, "set_multinomial(0) restores the per-fit object")
        assert not np.array_equal(multi["xopt"], ovr["xopt"])
        # folds or groups with the model set, in either order
        obj.set_multinomial(3)
        with pytest.raises(gpu.AdmmError, match="multinomial") as e:
            obj.set_folds(np.arange(SMALL[0]) % 3, np.zeros(K, dtype=np.int32))
        assert e.value.code == L.E_UNSUPPORTED
        with pytest.raises(gpu.AdmmError, match="multinomial") as e:
            obj.set_groups([SMALL[1]])
        assert e.value.code == L.E_UNSUPPORTED
        obj.set_multinomial(0)
        obj.set_groups([SMALL[1]])
        with pytest.raises(gpu.AdmmError, match="groups") as e:
            obj.set_multinomial(3)
        assert e.value.code == L.E_UNSUPPORTED
        obj.set_groups(None)
        obj.set_folds(np.arange(SMALL[0]) % 3, np.zeros(K, dtype=np.int32))
        with pytest.raises(gpu.AdmmError, match="folds") as e:
            obj.set_multinomial(3)
        assert e.value.code == L.E_UNSUPPORTED
        obj.set_folds(None, None)
        for bad in (1, 11, -2):
            with pytest.raises(gpu.AdmmError, match="classes") as e:
                obj.set_multinomial(bad)
            assert e.value.code == L.E_INVALID
        with pytest.raises(gpu.AdmmError, match="last chunk") as e:
            obj.set_multinomial(4)  # K = 6 is no multiple of 4
        assert e.value.code == L.E_INVALID
    finally:
        obj.close()
        fresh.close()
    # a row with two +1 labels, a model with two lambdas, a hinge fit
    m = SMALL[0]
    ELL = np.full((m, 3), -1.0, order="F")
    for k in range(3):
        ELL[c["y"] == k, k] = 1.0
    two = ELL.copy(order="F")
    two[17, :] = (1.0, 1.0, -1.0)
    for make, match in ((lambda: gpu.SparseL1Classifier(c["D"], two, [0.1] * 3), "row 17 carries 2"),
                        (lambda: gpu.SparseL1Classifier(c["D"], ELL, [0.1, 0.1, 0.2]), "slot 2 differs from slot 0"),
                        (lambda: gpu.SparseL1Classifier(c["D"], ELL, [0.1] * 3, ["logistic", "hinge", "logistic"]),
                         "slot 1 does not carry the logistic loss"),
                        (lambda: gpu.SparseL1Classifier(c["D"], ELL[:, :1], [0.1] * 3), "one label column per fit")):
        o = make()
        try:
            with pytest.raises(gpu.AdmmError, match=match) as e:
                o.set_multinomial(3)
            assert e.value.code == L.E_INVALID
        finally:
            o.close()


def test_the_tester_and_the_probabilities(gpu):
    test = gpu.testers.multinomialtest(seed=0)
    print({k: test[k] for k in ("objopt", "zeroobj", "accuracy", "df", "steps", "cg_capped_updates")})
    assert test["failed"] == 0
    p = gpu.multinomial_proba(test["D"], test["results"]["xopt"])
    assert p.shape == (test["D"].shape[0], 4) and np.all(p >= 0)
    assert np.max(np.abs(p.sum(axis=1) - 1.0)) <= 1e-14


def test_refusals_reach_no_device_work(gpu):
    c = R.case(gpu, SMALL, 3)
    with pytest.raises(ValueError, match="11 distinct classes"):
        gpu.multinomial(c["D"], np.arange(SMALL[0]) % 11, 0.1)
    with pytest.raises(ValueError, match="options.foldid"):
        gpu.multinomial(c["D"], c["y"], 0.1, dict(foldid=np.zeros(SMALL[0])))
