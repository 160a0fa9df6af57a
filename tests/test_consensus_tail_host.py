"""CPU-side checks behind tests/test_gpu_consensus_tail.py: the restatement of one consensus-lasso tail
(tests/consensus_restated.py) against the oracle's own consensus closures, the q identity the sharded run rests on,
that the rounding bound of the GPU tests leaves a float64 evaluation room, and that admm_op_consensus_tail refuses bad
arguments on the host and has no CPU fallback."""
import numpy as np
import pytest

import consensus_restated as CR
from oracle import proxops_ref

LD = np.longdouble


def _oracle_steps(iters=4, N=4, n=48, rows_per_slice=60, rho=1.3, seed=5):
    """the oracle's closures for `iters` iterations; per iteration what went in (x_k, u_k, xave, admm's u) and what
    came out (z, u_k, xave, ubar, lassonorms)"""
    rng = np.random.default_rng(seed)
    D = rng.standard_normal((N * rows_per_slice, n))
    s = rng.standard_normal(N * rows_per_slice)
    lam = 0.1 * float(np.max(np.abs(D.T @ s)))
    args = {"D": D, "s": s, "lambda": lam, "slices": [rows_per_slice] * N, "rho": rho}
    xmin, zmin, extra = proxops_ref.getproxops("LASSO", dict(args, parallel=1))
    st, xi, ui = extra["_state"], extra["_xi"], extra["_ui"]
    Dts = np.stack([D[k * rows_per_slice:(k + 1) * rows_per_slice].T @ s[k * rows_per_slice:(k + 1) * rows_per_slice]
                    for k in range(N)])
    steps, u_admm = [], np.zeros(n)
    for _ in range(iters):
        xmin(None, None, None, rho)
        before = dict(X=np.stack(xi), U=np.stack(ui), xave=st["xave"].copy(), ubar=u_admm.copy())
        zmin(None, None, None, rho)
        ub = extra["altu"](None, None, None, None)
        v = extra["specialnorms"](None, None, None, rho)
        after = dict(z=st["z"].copy(), U=np.stack(ui), xave=st["xave"].copy(), ubar=ub.copy(), v0=v[0], v1=v[1])
        steps.append((before, after))
        u_admm = ub
    return steps, Dts, rho, lam, N


def _rel(got, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - ref)) / max(np.max(np.abs(ref)), LD(1e-300)))


def _restated_vs_oracle(split):
    """largest difference, relative to the largest entry of each quantity, over 4 iterations"""
    steps, Dts, rho, lam, N = _oracle_steps()
    worst = 0.0
    for before, after in steps:
        if not split:
            r = CR.consensus_tail(before["X"], before["U"], Dts, before["xave"], before["ubar"], rho, lam, N,
                                  center=before["xave"])
            Unew, q = r["U"], r["q"]
            assert _rel(r["S_R2"], after["v0"]) < 1e-13  # the direct sum of the local slices IS lassonorms' first value
        else:  # Ntot = 4 as 2 + 2: each half sees the other's sums as `remote`; q is the only sum that adds up
            halves = []
            for a, b in ((slice(0, 2), slice(2, 4)), (slice(2, 4), slice(0, 2))):
                remote = np.stack([before["X"][b].astype(LD).sum(axis=0), before["U"][b].astype(LD).sum(axis=0)])
                halves.append(CR.consensus_tail(before["X"][a], before["U"][a], Dts[a], before["xave"], before["ubar"],
                                                rho, lam, N, remote=remote, center=before["xave"]))
            r = halves[0]
            for name in ("z", "xave", "ubar"):  # replicated state: the same on both halves
                assert _rel(halves[1][name], r[name]) < 1e-18
            Unew = np.concatenate([halves[0]["U"], halves[1]["U"]])
            q = halves[0]["q"] + halves[1]["q"]
        v0 = q - N * r["S_G2"]  # lassonorms' first value through the identity of the sharded run
        v1 = N * LD(rho) ** 2 * r["S_G2"]
        worst = max(worst, _rel(r["z"], after["z"]), _rel(Unew, after["U"]), _rel(r["xave"], after["xave"]),
                    _rel(r["ubar"], after["ubar"]), _rel(v0, after["v0"]), _rel(v1, after["v1"]))
    return worst


@pytest.mark.parametrize("split", [False, True], ids=["one-rank", "two-plus-two"])
def test_restatement_matches_the_oracle_closures(split):
    """The long-double restatement against oracle.getproxops("LASSO", ..., parallel) on 4 slices of 60 x 48, 4
    iterations: each iteration's x_k, u_k go in, the next z, u_k, xave, ubar and both lassonorms values come out (the
    first one through q - N*||xave - c||^2).  The oracle is float64 NumPy, the restatement the more exact side; the
    difference is the oracle's rounding.  Measured, relative to the largest entry of each quantity: 4.607e-16 as one
    rank, 4.607e-16 split 2 + 2 through `remote`.  Asserted: ten times that."""
    worst = _restated_vs_oracle(split)
    print(f"restatement vs oracle (split={split}): {worst:.3e}")
    assert worst <= 4.607e-15


def test_q_identity_on_the_restatement():
    """sum_k ||x_k - xave||^2 = q - N*||xave - c||^2 (consensus.hip) for any centre c: exact algebra, so the long-double
    restatement obeys it to its own rounding"""
    case = CR.make_case(0, 5, 300, "real", seed=3)
    for center in (case["xave"], np.zeros(300), 3.0 + case["ubar"]):
        r = CR.consensus_tail(case["X"], case["U"], case["Dts"], case["xave"], case["ubar"], case["rho"], case["lam"], 5,
                              center=center)
        dc2 = CR.slot_sums(case["X"], r["xave"], center, r["ubar"], case["ubar"])["S_G2"]  # ||xave - c||^2
        assert abs(r["S_R2"] - (r["q"] - 5 * dc2)) <= 1e-17 * r["q"]


def _all_cases():
    shapes = CR.F2_K_SWEEP + CR.F2_N_SWEEP + CR.F2_ROUND2 + CR.F1_SHAPES + CR.F0_SHAPES
    for form, K, n in shapes:
        for kind in ("int", "real"):
            yield CR.make_case(form, K, n, kind)
    yield CR.make_case(*CR.F2_BENCH, "int")
    for form in (0, 1):
        for kind in ("int", "real"):
            yield CR.make_case(form, 3, 1537, kind, Ntot=7)


def test_float64_in_kernel_order_stays_within_half_the_gpu_bound():
    """The GPU tests bound z, U, Y, xave and ubar by 16 * 2^-53 * operand scale.  A float64 NumPy evaluation in the
    kernels' order (consensus_restated.kernel_order_float64, x_k correctly rounded) must use at most half of that on
    every case the GPU tests run -- otherwise the bound would be a statement about rounding luck.  Measured: the worst
    ratio over all cases is 0.359 of the bound (Y of the integer case form 0, K = 17, n = 70001)."""
    worst = ("", 0.0)
    for case in _all_cases():
        X = case["X"] if case["form"] == 0 else CR.assemble(case["rows"])[0]
        args = (X, case["U"], case["Dts"], case["xave"], case["ubar"], case["rho"], case["lam"], case["Ntot"])
        ref = CR.consensus_tail(*args, remote=case["remote"], sums=False)
        got = CR.kernel_order_float64(*args, remote=case["remote"])
        for name, ratio in CR.vector_ratios(case, got, ref, X).items():
            assert ratio <= 0.5, (case["form"], case["K"], case["n"], case["kind"], name, ratio)
            if ratio > worst[1]:
                worst = (f"form {case['form']} K {case['K']} n {case['n']} {case['kind']} {name}", ratio)
        for i, target in case["kinks"].items():  # on the kink: zero with the sign of v
            assert got["z"][i] == 0 and ref["z"][i] == 0 and np.signbit(got["z"][i]) == (target < 0)
    print("worst ratio to the 16-rounding bound:", worst)


# ---------------------------------------------------------------------------------------------- argument rejection
def _tail_call(ap):
    """call(**overrides) -> rc: admm_op_consensus_tail with valid small arguments unless overridden (the pattern of
    _dense_op_calls in test_abi_and_host.py); a pointer override of None passes NULL"""
    L, dp = ap._lib.load(), ap._lib.as_dp
    n, K = 5, 2
    P = CR.partial_row_count(n)
    bufs = dict(rows=np.ones((K, P, n)), X=np.ones((K, n)), U=np.ones((K, n)), Dts=np.ones((K, n)), xave=np.ones(n),
                ubar=np.ones(n), remote=np.ones((2, n)), Y=np.zeros((K, n)), sums=np.zeros((2, n)), z=np.zeros(n),
                xaveprev=np.zeros(n), slots=np.zeros(5), q=np.zeros(1))

    def call(form=1, n=n, K=K, Ntot=K, rho=1.0, lam=0.5, with_q=0, **ptrs):
        a = {k: dp(v) for k, v in bufs.items()}
        a["remote"] = None
        a.update(ptrs)
        if a.get("remote") == "given":
            a["remote"] = dp(bufs["remote"])
        return L.admm_op_consensus_tail(form, n, K, Ntot, rho, lam, a["rows"], a["X"], a["U"], a["Dts"], a["xave"],
                                        a["ubar"], a["remote"], with_q, a["Y"], a["sums"], a["z"], a["xaveprev"],
                                        a["slots"], a["q"])

    return call, bufs


def test_consensus_tail_rejects_bad_arguments_before_touching_the_device(ap):
    """E_INVALID for null pointers, bad sizes and bad selectors -- decided on the host, so the answer is the same with
    and without a device"""
    call, _keep = _tail_call(ap)
    bad = [dict(form=-1), dict(form=3), dict(n=0), dict(K=0), dict(Ntot=1), dict(rho=0.0), dict(rho=-1.0),
           dict(rho=float("nan")), dict(rho=float("inf")), dict(lam=-1.0), dict(lam=float("nan")), dict(with_q=2),
           dict(with_q=-1), dict(rows=None), dict(form=2, rows=None), dict(X=None), dict(U=None), dict(Dts=None),
           dict(xave=None), dict(ubar=None), dict(Y=None), dict(sums=None), dict(z=None), dict(xaveprev=None),
           dict(slots=None), dict(with_q=1, q=None), dict(form=0, with_q=1, q=None),
           dict(form=2, K=17, Ntot=17), dict(form=2, remote="given", Ntot=3), dict(form=2, with_q=1),
           dict(K=2 ** 31 - 1, Ntot=2 ** 31 - 1, n=2 ** 40)]
    for kw in bad:
        assert call(**kw) == ap._lib.E_INVALID, kw
    assert "admm_op_consensus_tail" in ap._lib.EXPORTED_SYMBOLS


def test_consensus_tail_has_no_cpu_fallback(ap):
    """valid arguments: the result of a device, or E_DEVICE -- never a host computation"""
    call, _keep = _tail_call(ap)
    expected = ap._lib.OK if ap._lib.device_count() > 0 else ap._lib.E_DEVICE
    for kw in (dict(form=0, rows=None), dict(form=1), dict(form=2), dict(form=0, with_q=1),
               dict(form=1, Ntot=3, remote="given", with_q=1), dict(form=1, q=None)):
        assert call(**kw) == expected, kw
    if expected != ap._lib.OK:
        assert b"no CPU fallback" in ap._lib.load().admm_last_error()
