#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X ADMM engine (driver contract: see DESIGN.md).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Workload (BASELINE.json configs[1]): lasso.m on synthetic dense D 100000 x 10000 fp64, rho = 1,
lassotest.m:109-122 recipe (seed 1), fixed work via the reference's own switch domaxiters=1
(admm.m:59, 711).  A "step" is one ADMM iteration (admm.m:496-743) with D, the cached factor
and all iterates resident in HBM.  With N > 1 the SAME problem is row-sharded over the ranks
(slicemaker(0, N, m), errorcheck.m:249-259) -> strong scaling.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the headline (value, ms_per_step).
--full adds everything else: the x-solve roofline (HIP events, a run of its own), the side legs,
the other BASELINE configs, the all-reduce latencies (N > 1), the CPU baseline and the parity check.
--dump-outputs DIR writes what the timed run returned (xopt, zopt, uopt and the residual histories
of its K iterations, fp64) as DIR/<name>.npy; the inputs are seeded, so runs are comparable.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured float4 copy)
_DEV = "cuda"  # device of the torch tensors used for rendezvous collectives ("cpu" in --one-gpu rehearsals)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--cols", type=int, default=10000)
    ap.add_argument("--xsolve", default="inverse", choices=["trsv", "inverse"])
    ap.add_argument("--transport", default="rccl", choices=["rccl", "shm", "p2p"],
                    help="rccl: ncclAllReduce on the engine's stream; p2p: the engine's one-shot peer-to-peer all-reduce "
                         "(one kernel per rank, for the loop's 80-240 KB payloads); shm: host-staged (tests)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the objevals=1 and A-streaming side measurements")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--parity-iters", type=int, default=25,
                    help="iterations of the headline problem compared per iteration with the oracle (cpu_baseline leg)")
    ap.add_argument("--cpu-factor", default="own", choices=["own", "gpu"],
                    help="own: the CPU baseline forms D'D and its Cholesky factor itself (lasso.m:160-176, timed as "
                         "its setup); gpu: it takes the factor the device built")
    ap.add_argument("--one-gpu", action="store_true",
                    help="rehearsal on a single-GPU box: every rank uses HIP device 0, torch.distributed runs "
                         "over gloo and the engine over the shm transport (RCCL refuses two ranks on one device)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: roofline, side legs, other configs, all-reduce latencies, CPU baseline "
                         "and parity (the --no-* switches above trim this)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the timed run's results (xopt, zopt, uopt, pnorm, dnorm, perr, derr; fp64) as "
                         "DIR/<name>.npy")
    a = ap.parse_args(argv)
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    return a


def dist_setup(one_gpu=False):
    """One process per GPU (torch.distributed, backend nccl == RCCL).  Returns (rank, world, local, dist|None)."""
    global _DEV
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world == 1:
        return 0, 1, 0, None
    import torch
    import torch.distributed as dist

    if one_gpu:
        _DEV = "cpu"
        dist.init_process_group(backend="gloo")
        return rank, world, 0, dist
    torch.cuda.set_device(local)
    dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
    return rank, world, local, dist


def max_over_ranks(dist, value, device=None):
    if dist is None:
        return float(value)
    import torch

    t = torch.tensor([float(value)], dtype=torch.float64, device=device or _DEV)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def sync_all(dist):
    if dist is not None:
        import torch

        dist.barrier()
        if _DEV == "cuda":
            torch.cuda.synchronize()


def timed_run(eng, dist, steps, **kw):
    """barrier + sync, EXACTLY `steps` iterations, sync + barrier; MAX over ranks."""
    sync_all(dist)
    t0 = time.perf_counter()
    s = eng.run(maxiters=steps, domaxiters=1, record_history=0, **kw)  # returns after its stream drained
    sync_all(dist)
    dt = max_over_ranks(dist, time.perf_counter() - t0)
    assert s.steps == steps, (s.steps, steps)
    return dt, s


def make_problem(ap_mod, dist, m, n, lo, hi):
    """lassotest.m:109-122 at full size; each rank keeps only its rows [lo, hi) of D and s."""
    if dist is None:
        return ap_mod.synth.lasso_problem(seed=1, rows=m, cols=n)
    import torch

    p = ap_mod.synth.lasso_problem(seed=1, rows=m, cols=n, row_range=(lo, hi))
    g = torch.from_numpy(p["D"].T @ p["s"]).to(_DEV)  # lambda = 0.1*||D's||_inf needs the global D's
    dist.all_reduce(g)
    p["lam"] = 0.1 * float(g.abs().max().item())
    return p


def cpu_info():
    """CPU model, physical cores and BLAS vendor of the host the baseline runs on."""
    info = {"cpu_model": None, "physical_cores": None, "logical_cpus": os.cpu_count(), "blas": None}
    try:
        cores, phys, core = set(), None, None
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                key, _, val = line.partition(":")
                key, val = key.strip(), val.strip()
                if key == "model name" and info["cpu_model"] is None:
                    info["cpu_model"] = val
                elif key == "physical id":
                    phys = val
                elif key == "core id":
                    core = val
                elif not key and phys is not None and core is not None:
                    cores.add((phys, core))
                    phys = core = None
        if phys is not None and core is not None:
            cores.add((phys, core))
        info["physical_cores"] = len(cores) or None
    except OSError:
        pass
    try:
        from threadpoolctl import threadpool_info
        libs = [d for d in threadpool_info() if d.get("user_api") == "blas"]
        info["blas"] = "; ".join(f"{d.get('internal_api')} {d.get('version')} ({d.get('threading_layer', 'threads')}, "
                                 f"{d.get('num_threads')} threads, {d.get('architecture', '?')})" for d in libs) or None
    except Exception:
        pass
    return info


def _hist_err(got, ref):
    """max-norm relative error of one history (vectors: against the largest reference entry; scalars: entrywise)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape:
        return float("inf")
    if ref.ndim == 1:
        scale = np.maximum(np.abs(ref), 1e-12 + 1e-3 * np.max(np.abs(ref)))
        return float(np.max(np.abs(got - ref) / scale))
    return float(np.max(np.abs(got - ref)) / max(1e-300, np.max(np.abs(ref))))


def cpu_baseline(ap_mod, p, gpu_factor, gpu_hist, seconds, rho, own_factor=True):
    """The oracle's lasso loop (same algorithm and operation order as the reference: lasso.m:160-245, two triangular
    solves with the cached factor per iteration) on the host cores -- AFTER and OUTSIDE every timed GPU region.

    (1) setup as lasso.m:160-176 does it, on the host: D'D by BLAS, chol by LAPACK (`setup_seconds`, all cores);
    (2) parity: the oracle's first iterations with that factor -- nothing taken from the device -- against the
        histories the engine recorded for the same iterations (x, z, u, residuals, tolerances, objective);
    (3) the loop's rate, pinned to ONE BLAS thread (MATLAB applies the factor it stored sparse with single-threaded
        triangular solves, lasso.m:175-176) and with the whole pool."""
    import scipy.linalg as sla
    from oracle import admm as ref_admm
    from oracle import getproxops as ref_getproxops
    from threadpoolctl import threadpool_limits

    cores = ap_mod.synth.host_cores()
    D, s, lam = p["D"], p["s"], p["lam"]
    m, n = D.shape
    out = dict(value=None, unit="iterations/s", cores=1, kind="port", usable_cores=cores, **cpu_info())
    base = dict(A=1, At=1, m=n, nA=n, nB=n, B=-1, c=0, domaxiters=1, rho=rho)
    with threadpool_limits(limits=cores):
        t0 = time.perf_counter()
        Dts = D.T @ s
        if own_factor:
            factor = sla.cholesky(D.T @ D + rho * np.eye(n), lower=True, check_finite=False)  # lasso.m:168
            out["setup_seconds"] = time.perf_counter() - t0
            out["setup_note"] = f"D'D + chol on the host, BLAS pool limited to the {cores} usable cores (lasso.m:160-176)"
        else:
            factor = gpu_factor
        args = dict(D=D, Dts=Dts, L=factor, U=factor.T, m=m, n=n, parallel=0, rho=rho)
        args["lambda"] = lam
        minx, minz, _ = ref_getproxops("LASSO", args)
        if gpu_hist is not None:
            k = int(gpu_hist["steps"])
            obj = lambda x, z: 0.5 * float(np.sum((D @ x - s) ** 2)) + lam * float(np.sum(np.abs(z)))  # lasso.m:227
            ref = ref_admm(minx, minz, dict(base, maxiters=k, objevals=1, obj=obj))
            keys = ("xvals", "zvals", "uvals", "pnorm", "dnorm", "perr", "derr", "objevals")
            errs = {key: _hist_err(gpu_hist[key], ref[key]) for key in keys}
            out["_parity"] = {"iters": k, "max_rel": errs, "max": max(errs.values()), "tolerance": 1e-6,
                              "factor": "oracle's own (host BLAS/LAPACK)" if own_factor else "taken from the GPU setup",
                              "what": "engine histories of the first iterations (objevals=1) against the oracle's "
                                      "loop on the same D, s, lambda; max-norm relative error per history"}
        t0 = time.perf_counter()
        ref_admm(minx, minz, dict(base, maxiters=2))
        per = (time.perf_counter() - t0) / 2
    with threadpool_limits(limits=1):
        k1 = int(max(3, min(400, 0.6 * seconds / max(per, 1e-6))))
        r1 = ref_admm(minx, minz, dict(base, maxiters=k1))
    out.update(value=k1 / r1["runtime"],
               sample=f"{k1} iterations of the same {m}x{n} lasso loop (oracle restatement of admm.m:496-743 + "
                      f"getProxOps.m:1192-1206, SciPy/LAPACK triangular solves), BLAS limited to one thread; loop "
                      f"only, as results.runtime; restatement, not MATLAB")
    with threadpool_limits(limits=cores):
        k = int(max(3, min(300, 0.4 * seconds / max(per, 1e-6))))
        r = ref_admm(minx, minz, dict(base, maxiters=k))
    out["blas_pool"] = dict(value=k / r["runtime"], unit="iterations/s", threads=int(cores),
                            sample=f"{k} iterations with a BLAS pool of {int(cores)} threads: the triangular solves "
                                   f"barely thread, so this is about the single-thread number")
    return out


def profile_classes(eng, L, run):
    """HIP-event time of every kernel class (admm_engine_kernel_time) over one short extra run with profiling on --
    separate from the timed run, so the event records never sit inside a leg's timing."""
    eng.set_profiling(True)
    run()
    eng.set_profiling(False)
    names = {L.K_XSOLVE: "xsolve", L.K_GEMV_N: "gemv_n", L.K_GEMV_T: "gemv_t", L.K_PROX: "prox", L.K_FINALIZE: "finalize"}
    out = {}
    for k, name in names.items():
        ms, cnt = eng.kernel_time(k)
        if cnt:
            out[name] = {"avg_ms": ms / cnt, "launch_groups": cnt}
    return out


def leg_roofline(kernel, alg_bytes, avg_ms, bound="hbm", **extra):
    gbs = alg_bytes / (avg_ms * 1e-3) / 1e9 if avg_ms else None
    return dict({"bound": bound, "kernel": kernel, "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": avg_ms,
                 "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                 "frac": gbs / HBM_PEAK_GBS if gbs else None}, **extra)


def other_configs(ap, L, device, steps):
    """BASELINE.json configs 3 and 5 on one GPU (side lines; the headline stays config 2)."""
    res = {}
    # config 5: total variation, 1-D signal of length 4096^2 (the reference's TV is 1-D: totalvariation.m:127)
    n = 4096 * 4096
    p = ap.synth.tv_problem(seed=1, n=n)
    tv = ap.Engine(L.PROB_TOTALVARIATION, s=p["s"], lam=1.0, nvec=n, device=device)
    k = max(300, steps)  # 0.07 s of steady state (a 20-iteration timing is mostly ramp-up)
    tv.run(maxiters=20, domaxiters=1, record_history=0)
    t0 = time.perf_counter()
    s = tv.run(maxiters=k, domaxiters=1, record_history=0)
    dt = time.perf_counter() - t0
    passes = 3  # direct iteration kernel on the compact state v = z + u: reads s, v; writes v (5 up to r2i: z and u apart)
    res["totalvariation_16777216"] = {"iters_per_s": s.steps / dt, "ms_per_step": dt / s.steps * 1e3,
                                      "algorithmic_GB_per_iter": passes * 8.0 * n / 1e9,
                                      "achieved_GBs": passes * 8.0 * n * s.steps / dt / 1e9,
                                      "frac": passes * 8.0 * n * s.steps / dt / 1e9 / HBM_PEAK_GBS}
    cls = profile_classes(tv, L, lambda: tv.run(maxiters=64, domaxiters=1, record_history=0))
    res["totalvariation_16777216"]["kernel_classes"] = cls
    if "xsolve" in cls:
        res["totalvariation_16777216"]["roofline"] = leg_roofline(
            "tv_direct_kernel (one launch per iteration: x-solve, z/u update on the compact state, partial norms)",
            passes * 8.0 * n, cls["xsolve"]["avg_ms"])
    tv.close()
    # config 5 as literally written: anisotropic TV of a 4096 x 4096 IMAGE, no cached factor -- an engine-side
    # extension (the reference's solver is 1-D); own oracle, see tests/test_gpu_tv2d.py.  Two x-updates:
    # the direct spectral solve (2-D DCT, dct.hip; the default for power-of-two sides) and warm-started CG.
    hw = 4096
    rng = np.random.default_rng(1)
    img = np.zeros((hw, hw))
    img[hw // 5:hw // 2, hw // 6:hw // 2] = 2.0
    img[hw // 3:4 * hw // 5, hw // 3:5 * hw // 6] += 1.0
    img += rng.standard_normal((hw, hw))
    npix = hw * hw
    flat = np.asfortranarray(img).reshape(-1, order="F")
    for tag, xs, k2 in (("", L.XSOLVE_AUTO, max(200, steps)), ("_cg", L.XSOLVE_CG, max(10, steps // 20))):
        tv2 = ap.Engine(L.PROB_TV2D, s=flat, lam=1.0, shape=(hw, hw), xsolve=xs, device=device)
        tv2.run(maxiters=2, domaxiters=1, record_history=0)
        t0 = time.perf_counter()
        s2 = tv2.run(maxiters=k2, domaxiters=1, record_history=0)
        dt2 = time.perf_counter() - t0
        inner = float(tv2.fetch(L.F_CG_ITERS, 1)[0]) / s2.steps
        if xs == L.XSOLVE_CG:
            # doubles per ADMM iteration: CG start 12N + fused z/u/dual/rhs pass 7N + 10N per inner iteration
            # (fused direction + stencil: reads r, p, writes p, q; update: reads x, p, r, q, writes x, r)
            gb = (19.0 + 10.0 * inner) * 8.0 * npix / 1e9
            extra = {"x_update": "cg", "cg_inner_iters_per_step": inner, "cg_tol": 1e-11}
        else:
            # three launches: row stage 2N (transformed right-hand side -> scratch image), inverse column DCT 2N, and the
            # fused z/u/dual pass on the compact state v = z + u whose right-hand side goes through the forward column
            # DCT inside the kernel: 4N read (x, v, s) + 3N written (v, transformed next rhs) = 11N.  (Round 2 and the
            # start of round 3: b written and read back, 13N in four launches; up to r2i 17N; round 1: 21N.)
            gb = 11.0 * 8.0 * npix / 1e9
            extra = {"x_update": "dct",
                     "frac_in_the_13N_unit_of_round_2": 13.0 * 8.0 * npix / 1e9 * s2.steps / dt2 / HBM_PEAK_GBS}
        res["totalvariation2d_4096x4096" + tag] = dict(
            {"iters_per_s": s2.steps / dt2, "ms_per_step": dt2 / s2.steps * 1e3, "algorithmic_GB_per_iter": gb,
             "achieved_GBs": gb * s2.steps / dt2, "frac": gb * s2.steps / dt2 / HBM_PEAK_GBS}, **extra)
        if xs != L.XSOLVE_CG:
            cls = profile_classes(tv2, L, lambda: tv2.run(maxiters=32, domaxiters=1, record_history=0))
            res["totalvariation2d_4096x4096" + tag]["kernel_classes"] = cls
            if "xsolve" in cls and "prox" in cls:
                res["totalvariation2d_4096x4096" + tag]["roofline"] = {
                    "spectral_solve": leg_roofline("tv2d_rows_coop + dct_cols_inverse (2 launches)",
                                                   4.0 * 8.0 * npix, cls["xsolve"]["avg_ms"], bound="hbm+infinity_cache"),
                    "fused_pass": leg_roofline("tv2d_fused_dct_kernel (z/u update, dual stencils, next right-hand "
                                               "side -> forward column DCT in LDS)", 7.0 * 8.0 * npix,
                                               cls["prox"]["avg_ms"])}
        tv2.close()
    return res


def consensus_leg(ap, L, a, dist, p, rho, device, comm, rank, world, m_global, xs):
    """BASELINE config 4: consensus lasso over the 8 row slices slicemaker(0, 8, m) gives (lasso.m:196-208,
    getProxOps.m:383-442, 1217-1343) -- the SAME 8-slice problem at every N: rank r holds 8/N local slices, each with its
    own x_k, u_k and cached factor; per iteration 8/N lower-triangle x-solves per GPU and (N > 1) ONE all-reduce of
    [sum x_k; sum u_k; q] = 2n + 1 doubles."""
    n = p["D"].shape[1]
    sl8 = [int(v) for v in ap.errorcheck.slicemaker(0, 8, m_global)]
    if 8 % world != 0:
        return {"skipped": f"8 slices do not divide over {world} ranks"}
    per = 8 // world
    mine = sl8[rank * per:(rank + 1) * per]
    assert sum(mine) == p["D"].shape[0], (mine, p["D"].shape)
    cons = ap.Engine(L.PROB_LASSO_CONSENSUS, D=p["D"], s=p["s"], lam=p["lam"], rho=rho, slices=mine, xsolve=xs,
                     device=device, comm=comm)
    k = max(50, a.steps // 4)
    timed_run(cons, dist, 3, rho=rho, stopcond="both")
    dt, _ = timed_run(cons, dist, k, rho=rho, stopcond="both")
    cons.set_profiling([L.K_XSOLVE, L.K_PROX])
    timed_run(cons, dist, 20, rho=rho, stopcond="both")
    cons.set_profiling(False)
    xs_ms, xs_cnt = cons.kernel_time(L.K_XSOLVE)
    px_ms, px_cnt = cons.kernel_time(L.K_PROX)
    info = cons.info()
    gb_gpu = per * 4.0 * n * (n + 1) / 1e9  # per GPU: 8/N slices x lower triangle of an n x n inverse
    xs_avg = xs_ms / max(1, xs_cnt)
    out = {"workload": f"consensus lasso, 8 row slices of {sl8[0]} x {n} in total, {per} per GPU (config 4)",
           "slices_total": 8, "slices_per_gpu": per, "iters_per_s": k / dt, "ms_per_step": dt / k * 1e3,
           "algorithmic_GB_per_iter_per_gpu": gb_gpu, "achieved_GBs_per_gpu": gb_gpu * k / dt,
           "frac": gb_gpu * k / dt / HBM_PEAK_GBS,
           "collectives_per_iter": 1 if world > 1 else 0, "allreduce_doubles_per_iter": (2 * n + 1) if world > 1 else 0,
           "roofline": {"bound": "hbm+infinity_cache", "kernel": "symv_lower_batch_fin_kernel (the local slices' x-solves "
                        "as one launch)", "avg_launch_ms": xs_avg, "launches": xs_cnt,
                        "algorithmic_bytes_per_launch": gb_gpu * 1e9,
                        "achieved": gb_gpu / (xs_avg * 1e-3) if xs_cnt else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": gb_gpu / (xs_avg * 1e-3) / HBM_PEAK_GBS if xs_cnt else None,
                        "llc_resident_bytes": info["xsolve_cacheable_bytes"],
                        "tail_ms_per_iter": dt / k * 1e3 - xs_avg if xs_cnt else None,
                        "update_kernels_avg_ms": px_ms / max(1, px_cnt)},
           "setup_seconds": max_over_ranks(dist, cons.setup_seconds)}
    cons.close()
    return out


def _svm_configs(ap, L, device, res):
    # config 3: linear SVM, hinge, MNIST-shaped synthetic pixels (image files are absent from the reference)
    for m in (6000, 60000):
        # images: synthetic (the reference tree holds no MNIST image file); labels: the reference's own
        # examples/MNIST/train-labels.idx1-ubyte (tests/golden/mnist/), digit 0 against the rest (mnistsvm.m:133-142)
        q = ap.synth.mnist_like_problem(seed=1, m=m, n=400, digit=0, labels=ap.synth.reference_mnist_labels("train"))
        svm = ap.Engine(L.PROB_LINEARSVM, D=q["D"], ell=q["ell"], Cval=q["C"], xsolve=L.XSOLVE_INVERSE, device=device)
        kw = dict(maxiters=1000, domaxiters=1, record_history=0, nodualerror=1, stopcond="both",
                  x0=q["x0"], z0=q["z0"], u0=q["u0"])  # unwrappedadmm.m:87-92
        svm.run(**dict(kw, maxiters=20))
        t0 = time.perf_counter()
        s = svm.run(**kw)
        dt = time.perf_counter() - t0
        mb = 16.0 * m * 400 / 1e6
        cls = profile_classes(svm, L, lambda: svm.run(**dict(kw, maxiters=64)))
        two_launch = bool(svm.info()["unwrapped_fused"])
        one_pass = not two_launch and "gemv_n" not in cls  # (unwrapped.hip: ad_onepass_kernel launches no D*x of its own)
        res[f"linearsvm_{m}x400"] = {"iters_per_s": s.steps / dt, "ms_per_step": dt / s.steps * 1e3,
                                     "algorithmic_MB_per_iter": mb,
                                     "achieved_GBs": mb * 1e6 * s.steps / dt / 1e9,
                                     "frac": mb * 1e6 * s.steps / dt / 1e9 / HBM_PEAK_GBS,
                                     "two_launch_iteration": two_launch, "one_pass_iteration": one_pass,
                                     "note": ("D and pinv(D) (2 x %.0f MB) sit in the 256 MB Infinity Cache: latency-bound, "
                                              "the fraction is an effective rate" % (mb / 2)) if mb < 200 else
                                             ("the unit is the iteration's two products D*x and D'*(c + z - u) "
                                              "(2 x %.0f MB); the one-pass kernel READS D once per iteration (64-row "
                                              "blocks held in registers serve both products): in bytes actually moved "
                                              "the rate is half the figure" % (mb / 2)) if one_pass else
                                             ("D (%.0f MB) is read twice per iteration (D*x, D'*[..]) and only partly "
                                              "cache-resident: effective rate of both passes" % (mb / 2))}
        if one_pass:
            res[f"linearsvm_{m}x400"]["frac_of_bytes_read"] = 0.5 * res[f"linearsvm_{m}x400"]["frac"]
        res[f"linearsvm_{m}x400"]["kernel_classes"] = cls
        svm.close()


def _leg(name):
    """progress marker on stderr (one line per bench leg: locates a failure under a profiler)"""
    print(f"bench.py: leg {name}", file=sys.stderr, flush=True)


def side_engines(ap, L, a, dist, p, xs, local, comm, lo, hi, n, rho, world, out, m_global):
    """The A-streaming legs (lad.m, matrix-free lasso) on the same D, s, and configs 3 / 5 at N = 1."""
    _leg("a_streaming (lad)")
    # A-streaming iteration on the same D, s: lad.m (x = R'\(R\(D'(s+z-u))), z = soft(Dx+u-s)) --
    # exactly one D*x and one D'*[3 rhs] pass per iteration = the "A'(Ax-b)" unit, 16mn bytes,
    # row-sharded with ONE all-reduce per iteration when N > 1 (unwrappedadmm.m:96-141).
    lad = ap.Engine(L.PROB_LAD, D=p["D"], s=p["s"], xsolve=xs, device=local, comm=comm)
    k2 = max(40, a.steps // 4)
    timed_run(lad, dist, 2)
    lad.set_profiling([L.K_GEMV_N, L.K_GEMV_T])
    dt2, _ = timed_run(lad, dist, k2)
    lad.set_profiling(False)
    gn_ms, gn_cnt = lad.kernel_time(L.K_GEMV_N)
    gt_ms, gt_cnt = lad.kernel_time(L.K_GEMV_T)
    pair_ms = gn_ms / max(1, gn_cnt) + gt_ms / max(1, gt_cnt)
    rows_local = hi - lo
    gbs = 16.0 * rows_local * n / (pair_ms * 1e-3) / 1e9 if pair_ms > 0 else 0.0
    out["a_streaming"] = {"workload": "lad.m on the same D,s: D*x + D'*[s+z-u, dz, u] per iteration (16mn B), "
                                      "transpose reduction over the row shards",
                          "iters_per_s": k2 / dt2, "ms_per_step": dt2 / k2 * 1e3,
                          "AtAx_unit_ms": pair_ms, "AtAx_GBs_per_gpu": gbs, "AtAx_frac": gbs / HBM_PEAK_GBS,
                          "AtAx_traffic_bytes": out.get("_pmc_pair"),
                          "gemv_n_avg_ms": gn_ms / max(1, gn_cnt), "gemv_t_avg_ms": gt_ms / max(1, gt_cnt),
                          "setup_seconds": max_over_ranks(dist, lad.setup_seconds)}
    lad.close()

    # objevals=1 with the objective as the reference writes it, one extra D*x pass per iteration (obj_gram = -1)
    _leg("objevals1_literal")
    lg = ap.Engine(L.PROB_LASSO, D=p["D"], s=p["s"], lam=p["lam"], rho=rho, xsolve=xs, device=local, comm=comm,
                   obj_gram=-1)
    kg = max(50, a.steps // 4)
    timed_run(lg, dist, 2, rho=rho, objevals=1)
    lg.set_profiling([L.K_GEMV_N])
    dtg, _ = timed_run(lg, dist, kg, rho=rho, objevals=1)
    lg.set_profiling(False)
    gn_ms, gn_cnt = lg.kernel_time(L.K_GEMV_N)
    rows_local = hi - lo
    gbs = 8.0 * rows_local * n / (gn_ms / max(1, gn_cnt) * 1e-3) / 1e9 if gn_cnt else 0.0
    out["objevals1_literal"] = {"iters_per_s": kg / dtg, "ms_per_step": dtg / kg * 1e3,
                                "gemv_n_GBs_per_gpu": gbs, "gemv_n_frac": gbs / HBM_PEAK_GBS,
                                "gemv_n_avg_ms": gn_ms / max(1, gn_cnt),
                                "note": "one extra D*x pass (8mn B) per iteration, row-sharded when N > 1; timing "
                                        "includes the residual-norm kernel"}
    lg.close()

    # the same loop with the factor applied as the reference writes it, two triangular solves (trsv.hip): blocked
    # substitution with pre-inverted diagonal blocks -- K = ceil(n/2048) coarse blocks, 2K + 1 launches per pair, or
    # ONE block (the whole factor pre-inverted: two passes over inv(L), two launches) where the probe at create finds
    # that form as accurate as the K-block one; both read 8 n(n+1) bytes per pair
    if world == 1:
        _leg("xsolve_trsv")
        lt = ap.Engine(L.PROB_LASSO, D=p["D"], s=p["s"], lam=p["lam"], rho=rho, xsolve=L.XSOLVE_TRSV, device=local)
        ti = lt.info()
        kt = max(100, a.steps // 2)
        timed_run(lt, dist, 3, rho=rho)
        dtt, _ = timed_run(lt, dist, kt, rho=rho)
        out["xsolve_trsv"] = {"iters_per_s": kt / dtt, "ms_per_step": dtt / kt * 1e3,
                              "algorithmic_GB_per_iter": 8.0 * n * (n + 1) / 1e9,
                              "frac": 8.0 * n * (n + 1) * kt / dtt / 1e9 / HBM_PEAK_GBS,
                              "trsv_blocks": ti["trsv_blocks"],
                              "probe_err_one_block": ti["probe_err_trsv_one"],
                              "probe_err_blocked": ti["probe_err_trsv"],
                              "note": "x = L'\\(L\\y) as getProxOps.m:1200 writes it: blocked substitution with "
                                      "pre-inverted diagonal blocks; trsv_blocks = 1: the whole factor is the one "
                                      "block (w = inv(L) y, x = inv(L)' w: two passes over one tile-packed triangle), "
                                      "kept because its probe error matches the K-block form's; same iterates as the "
                                      "headline"}
        lt.close()

    # matrix-free lasso (xsolve = cg): same iterates as the cached-factor loop (inner tolerance
    # 1e-10), every inner iteration one A'(A p) unit, nothing n x n stored
    _leg("matrix_free (cg)")
    mf = ap.Engine(L.PROB_LASSO, D=p["D"], s=p["s"], lam=p["lam"], rho=rho, xsolve=L.XSOLVE_CG, device=local,
                   comm=comm, cg_tol=1e-10)
    k3 = max(10, a.steps // 40)
    timed_run(mf, dist, 1, rho=rho)
    mf.set_profiling([L.K_GEMV_N, L.K_GEMV_T])
    dt3, _ = timed_run(mf, dist, k3, rho=rho)
    mf.set_profiling(False)
    inner = float(mf.fetch(L.F_CG_ITERS, 1)[0])
    gn_ms, _ = mf.kernel_time(L.K_GEMV_N)
    gt_ms, _ = mf.kernel_time(L.K_GEMV_T)
    # operator applications that did work: one per inner iteration + the initial residual of every solve
    # (launches enqueued past convergence are no-ops and must not be counted as units)
    pair_ms = (gn_ms + gt_ms) / max(1.0, inner + k3)
    gbs = 16.0 * (hi - lo) * n / (pair_ms * 1e-3) / 1e9 if pair_ms > 0 else 0.0
    out["matrix_free"] = {"workload": "lasso, x-update by warm-started CG on (D'D + rho I), tol 1e-10",
                          "iters_per_s": k3 / dt3, "ms_per_step": dt3 / k3 * 1e3,
                          "inner_iters_per_step": inner / k3, "AtAx_unit_ms": pair_ms,
                          "AtAx_GBs_per_gpu": gbs, "AtAx_frac": gbs / HBM_PEAK_GBS,
                          "setup_seconds": max_over_ranks(dist, mf.setup_seconds)}
    mf.close()

    _leg("consensus_lasso (config 4: 8 slices in total at every N)")
    rank = comm.rank if comm is not None else 0
    out["consensus_lasso"] = consensus_leg(ap, L, a, dist, p, rho, local, comm, rank, world, m_global, xs)
    if world > 1 and comm is not None and ((comm.transport == "rccl" and not a.one_gpu) or
                                           os.environ.get("ADMM_BENCH_P2P_LEG")):  # (the env: rehearsal of this leg)
        # the same leg over the engine's own one-shot peer-to-peer all-reduce (comm.hip: ADMM_COMM_P2P), with what the
        # payloads of the legs cost on it -- next to RCCL's numbers in config.communicator.allreduce_us.  Contained: this
        # transport has never run on real links in this repository's records; its polling is bounded (error, no hang)
        _leg("consensus_lasso over the one-shot P2P all-reduce")
        import threading

        def _give_up():  # this leg is the LAST thing an N > 1 run measures: the line so far is the result
            out["consensus_lasso_p2p"] = {"error": "the P2P leg did not finish within 90 s: abandoned"}
            out.pop("_pmc_pair", None)
            if rank == 0:
                print(json.dumps(out), flush=True)
            os._exit(0)

        watchdog = threading.Timer(90.0, _give_up)
        watchdog.daemon = True
        watchdog.start()
        try:
            from admm_project_amd import parallel as _par
            c2 = _par.init_from_torch(dist, device=local, transport="p2p")
            try:
                lat = {f"{cnt}_doubles": max_over_ranks(dist, c2.allreduce_latency_us(cnt, 50))
                       for cnt in (1, n, 2 * n + 1, 3 * n + 16)}
                leg = consensus_leg(ap, L, a, dist, p, rho, local, c2, rank, world, m_global, xs)
                leg["allreduce_us"] = lat
                out["consensus_lasso_p2p"] = leg
            finally:
                c2.close()
        except Exception as exc:
            out["consensus_lasso_p2p"] = {"error": repr(exc)}
        finally:
            watchdog.cancel()
    if world == 1:
        _leg("other_configs (tv, tv2d, svm)")
        out["other_configs"] = other_configs(ap, L, local, a.steps)
        _svm_configs(ap, L, local, out["other_configs"])
        # the same object under its round-2 name
        out["other_configs"][f"consensus_lasso_8x{m_global // 8}x{n}"] = out["consensus_lasso"]


def main():
    a = parse()
    rank, world, local, dist = dist_setup(a.one_gpu)
    if a.one_gpu and a.transport == "rccl":
        a.transport = "shm"  # (RCCL refuses two ranks on one device; p2p is fine with it)
    if world != a.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}; launch with torch.distributed.run",
                  file=sys.stderr)
        sys.exit(2)
    import admm_project_amd as ap
    from admm_project_amd import parallel

    L = ap._lib
    L.require_device()
    m, n = a.rows, a.cols
    rho = 1.0
    comm = None
    transport = None
    comm_report = {"ranks": 1, "transport": None}
    lo, hi = 0, m
    if dist is not None:
        transport = a.transport
        try:
            comm = parallel.init_from_torch(dist, device=local, transport=transport)
        except ap.AdmmError as exc:  # RCCL refused the topology: host-staged transport still measures the GPUs
            if rank == 0:
                print(f"bench.py: RCCL communicator failed ({exc}); falling back to the shm transport", file=sys.stderr)
            transport = "shm"
            comm = parallel.init_from_torch(dist, device=local, transport=transport)
        lo, hi = parallel.my_rows(m, comm)
        if 8 % world == 0:
            # config 4 is an 8-slice consensus problem at EVERY N: rank r owns slices [r*8/N, (r+1)*8/N) of
            # slicemaker(0, 8, m) (errorcheck.m:249-259) and, for every other leg, exactly those rows
            sl8 = [int(v) for v in ap.errorcheck.slicemaker(0, 8, m)]
            per = 8 // world
            lo = sum(sl8[:rank * per])
            hi = lo + sum(sl8[rank * per:(rank + 1) * per])
        # what the engine's communicator itself reports (a SCALE record is self-checking: ranks and transport)
        import ctypes as _C
        _r, _n, _t = _C.c_int(), _C.c_int(), _C.c_int()
        L.check(L.load().admm_comm_info(comm.handle, _C.byref(_r), _C.byref(_n), _C.byref(_t)))
        comm_report = {"ranks": _n.value, "rank0_sees": _r.value,
                       "transport": {L.COMM_RCCL: "rccl", L.COMM_SHM: "shm", L.COMM_P2P: "p2p"}[_t.value]}
        if a.full:
            # what one per-iteration exchange costs on the links this group really has (the payloads of the side legs)
            comm_report["allreduce_us"] = {f"{cnt}_doubles": max_over_ranks(dist, comm.allreduce_latency_us(cnt, 50))
                                           for cnt in (1, n, 2 * n + 1, 3 * n + 16)}

    t0 = time.perf_counter()
    p = make_problem(ap, dist, m, n, lo, hi)
    t_gen = time.perf_counter() - t0

    xs = {"trsv": L.XSOLVE_TRSV, "inverse": L.XSOLVE_INVERSE}[a.xsolve]
    eng = ap.Engine(L.PROB_LASSO, D=p["D"], s=p["s"], lam=p["lam"], rho=rho, xsolve=xs, device=local, comm=comm)
    setup_s = max_over_ranks(dist, eng.setup_seconds)

    # ---- headline: objevals = 0 ----------------------------------------------------------
    _leg("headline")
    timed_run(eng, dist, max(1, a.warmup), rho=rho)
    dt, s_head = timed_run(eng, dist, a.steps, rho=rho)
    value = a.steps / dt
    if a.dump_outputs:  # what a caller of this run receives; every run starts from x = z = u = 0
        k = int(s_head.steps)
        dumped = {"xopt": eng.fetch(L.F_XOPT, n), "zopt": eng.fetch(L.F_ZOPT, n), "uopt": eng.fetch(L.F_UOPT, n),
                  "pnorm": eng.fetch(L.F_PNORM, k), "dnorm": eng.fetch(L.F_DNORM, k),
                  "perr": eng.fetch(L.F_PERR, k), "derr": eng.fetch(L.F_DERR, k)}
        if rank == 0:
            os.makedirs(a.dump_outputs, exist_ok=True)
            for name, arr in dumped.items():
                np.save(os.path.join(a.dump_outputs, f"{name}.npy"), np.ascontiguousarray(arr, dtype=np.float64))
    out = {
        "metric": "ADMM iterations/sec (lasso 100k x 10k, fp64)", "value": value, "unit": "iterations/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"lasso.m cached-factor loop, D {m}x{n} fp64, rho=1, lassotest.m recipe seed=1, "
                               f"domaxiters=1, objevals=0, xsolve={a.xsolve}",
                   "rows": m, "cols": n, "rho": rho, "parallelism": f"rows{world}", "collective": transport,
                   "communicator": comm_report},
        "setup_seconds": setup_s, "datagen_seconds": t_gen,
    }
    if a.full:
        full_measurements(ap, L, a, dist, eng, p, out, dt, xs, local, comm, lo, hi, m, n, rho, world, rank)
    else:
        eng.close()
    if rank == 0:
        print(json.dumps(out))
    if comm is not None:
        comm.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def full_measurements(ap, L, a, dist, eng, p, out, dt, xs, local, comm, lo, hi, m, n, rho, world, rank):
    """--full: everything past the headline, on the same resident data (eng is closed on return)."""
    # only the dominant kernel class, every 4th iteration: K more steps with the event pairs in the stream
    _leg("roofline")
    eng.set_profiling([L.K_XSOLVE], stride=4)
    dt_ev, _ = timed_run(eng, dist, a.steps, rho=rho)
    eng.set_profiling(False)
    xs_ms, xs_cnt = eng.kernel_time(L.K_XSOLVE)
    if a.xsolve == "inverse":
        alg_bytes = 8.0 * n * (n + 1) / 2  # lower triangle of the symmetric inverse, read once
        kname = ("symv_lower_fin_kernel: x = inv(D'D+rho I) * y from the tile-packed lower triangle only (its first "
                 "168 MB stay in the Infinity Cache between iterations, the rest streams non-temporally; workgroup 0 "
                 "carries the previous iteration's finalize logic; the partial rows are summed by prox_fin_kernel)")
    else:
        alg_bytes = 8.0 * n * (n + 1)  # two triangular solves
        kname = "tri_step_kernel x 2K + tri_fold (x = L'\\(L\\y), blocked substitution, K coarse blocks)"
    # HBM bytes per launch from the committed PMC passes of this same script (profiles/r2_traffic.json, produced by
    # profiles/collect.sh + summarize.py; bench.py cannot run rocprofv3 on itself): valid for the default size
    traffic = None
    tj = {}
    for name in ("r3f_traffic.json", "r3e_traffic.json", "r3d_traffic.json", "r3c_traffic.json", "r3b_traffic.json", "r3_traffic.json", "r2_traffic.json", "r1_traffic.json"):
        tfile = os.path.join(ROOT, "profiles", name)
        if os.path.exists(tfile):
            with open(tfile) as fh:
                tj = json.load(fh)
            break

    def pmc_bytes(*prefixes):
        tot = 0.0
        for pre in prefixes:
            hit = [v for k, v in tj.items() if k.startswith(pre) and isinstance(v, dict)]
            if not hit:
                return None
            tot += hit[0].get("fetch_bytes_per_launch", 0.0) + hit[0].get("write_bytes_per_launch", 0.0)
        return tot

    if n == 10000 and m == 100000:
        traffic = (pmc_bytes("admm::symv_lower_fin_kernel") or pmc_bytes("void admm::symv_lower_kernel<true>")
                   if a.xsolve == "inverse" else None)
    xs_avg_ms = xs_ms / max(1, xs_cnt)
    achieved = alg_bytes / (xs_avg_ms * 1e-3) / 1e9 if xs_cnt else 0.0
    # The Infinity Cache's share, said out loud: the engine reads `llc` bytes of the matrix with default loads so that
    # they stay in the 256 MB last-level cache from one iteration to the next (symv.hip: split cache policy) and streams
    # the rest non-temporally.  `achieved` / `frac` are the effective rate of the kernel against the HBM peak;
    # `frac_hbm_only` prices only the bytes that can come from HBM itself.
    einfo = eng.info()
    llc = int(einfo["xsolve_cacheable_bytes"])
    streamed = int(einfo["xsolve_stream_bytes"])
    scale = alg_bytes / max(1.0, float(llc + streamed))  # tile padding: stored bytes -> algorithmic bytes
    hbm_est = streamed * scale if llc + streamed > 0 else alg_bytes
    hbm_only = hbm_est / (xs_avg_ms * 1e-3) / 1e9 if xs_cnt else 0.0
    out.update({
        "roofline": {"bound": "hbm+infinity_cache" if llc > 0 and streamed > 0 else "hbm", "achieved": achieved,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "kernel": kname,
                     "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": xs_avg_ms, "launches": xs_cnt,
                     "llc_resident_bytes": llc, "hbm_bytes_est": hbm_est, "achieved_hbm_only": hbm_only,
                     "frac_hbm_only": hbm_only / HBM_PEAK_GBS,
                     "traffic_source": "profiles/*_traffic.json (committed rocprofv3 --pmc passes of this script; the "
                                       "FETCH counter sits between L2 and the fabric and counts Infinity-Cache hits)"},
        "scaling_basis": {
            "value": "flat in N by design: the cached-factor lasso loop replicates x, z, u and the n x n factor on every "
                     "rank and exchanges nothing per iteration (D enters only the setup and the objective)",
            "strong_scaling_legs": ["a_streaming", "objevals1_literal", "matrix_free"],
            "per_gpu_bytes_per_iter": "16*(m/N)*n (a_streaming, matrix_free per inner iteration), 8*(m/N)*n "
                                      "(objevals1_literal)",
            "consensus_lasso": "the same 8-slice problem at every N, 8/N slices per GPU: per-GPU bytes 8/N * 4n(n+1)",
            "collectives_per_iter": {"headline": 0, "a_streaming": 1 if world > 1 else 0,
                                     "objevals1_literal": 1 if world > 1 else 0,
                                     "matrix_free": "1 per inner CG iteration" if world > 1 else 0,
                                     "consensus_lasso": 1 if world > 1 else 0},
            "allreduce_doubles": {"a_streaming": 3 * n + 16, "objevals1_literal": 1, "matrix_free": n,
                                  "consensus_lasso": 2 * n + 1}},
        "iters_per_s_without_event_timing": a.steps / dt,
        "iters_per_s_with_event_timing": a.steps / dt_ev,
        "achieved_hbm_GBs_whole_iteration": (alg_bytes + 8.0 * 21 * n) * a.steps / dt / 1e9,
    })

    if a.steps < 100:  # the driver's --steps 20 times 1.5 ms, of which 43 us are per-run fixed cost: also the 200-step rate
        dt200, _ = timed_run(eng, dist, 200, rho=rho)
        out["value_200"] = 200 / dt200
        out["ms_per_step_200"] = dt200 / 200 * 1e3

    # the same loop with the reference's histories on (admm.m:608-610 always records xvals/zvals/uvals)
    kh = max(20, min(a.steps, 200))
    eng.run(maxiters=3, domaxiters=1, record_history=1, rho=rho)
    sync_all(dist)
    t0h = time.perf_counter()
    sh = eng.run(maxiters=kh, domaxiters=1, record_history=1, rho=rho)
    sync_all(dist)
    dth = max_over_ranks(dist, time.perf_counter() - t0h)
    out["record_history1"] = {"iters_per_s": sh.steps / dth, "ms_per_step": dth / sh.steps * 1e3,
                              "note": "xvals/zvals/uvals written by the fused kernels into device buffers "
                                      "(admm.m:608-610); includes allocating 3 x n x maxiters doubles per run"}

    # ---- side measurements (same resident data) --------------------------------------------
    if not a.no_extras:
        _leg("objevals1")
        k1 = max(100, a.steps)
        timed_run(eng, dist, 5, rho=rho, objevals=1)  # first objevals batch: both objective forms, then the decision
        dt1, s1 = timed_run(eng, dist, k1, rho=rho, objevals=1)
        out["objevals1"] = {"iters_per_s": k1 / dt1, "ms_per_step": dt1 / k1 * 1e3,
                            "objective_form": "solve_identity" if int(getattr(s1, "obj_gram_used", 0)) else "literal",
                            "note": "lassotest.m:131 sets objevals=1.  Default (obj_gram = 0): the engine evaluates "
                                    "1/2*||D*x - s||^2 both literally (one D*x pass, 8mn B) and as 1/2*x'(y - rho*x) - x'D's "
                                    "+ 1/2*s's (y = the right-hand side x was solved from: G x = y - rho*x; summed by the "
                                    "element update, no extra pass) during the first batch and keeps the second form only "
                                    "if they agreed to 1e-11 relative"}

    factor = None
    gpu_hist = None
    if not a.no_cpu_baseline and world == 1:
        if a.cpu_factor == "gpu":
            factor = eng.fetch(L.F_FACTOR, n * n, (n, n))
        if a.parity_iters > 0:  # histories of the first iterations from x = z = u = 0, for the parity object
            kp = a.parity_iters
            sp_ = eng.run(maxiters=kp, domaxiters=1, record_history=1, rho=rho, objevals=1)
            gpu_hist = {"steps": int(sp_.steps),
                        "xvals": eng.fetch(L.F_XVALS, n * kp, (n, kp)), "zvals": eng.fetch(L.F_ZVALS, n * kp, (n, kp)),
                        "uvals": eng.fetch(L.F_UVALS, n * kp, (n, kp)), "pnorm": eng.fetch(L.F_PNORM, kp),
                        "dnorm": eng.fetch(L.F_DNORM, kp), "perr": eng.fetch(L.F_PERR, kp),
                        "derr": eng.fetch(L.F_DERR, kp), "objevals": eng.fetch(L.F_OBJEVALS, kp)}
    eng.close()

    if n == 10000 and m == 100000 and world == 1:  # PMC bytes of one D*x + one D'*[3 rhs] launch
        out["_pmc_pair"] = pmc_bytes("void admm::gemv_n_kernel", "void admm::gemv_t_kernel<3")
    if not a.no_extras:
        try:
            side_engines(ap, L, a, dist, p, xs, local, comm, lo, hi, n, rho, world, out, m)
        except Exception as exc:  # the side measurements must never cost the headline line
            out["extras_error"] = repr(exc)

    if not a.no_cpu_baseline and world == 1 and rank == 0:
        _leg("cpu_baseline + parity (host)")
        try:
            cb = cpu_baseline(ap, p, factor, gpu_hist, a.cpu_seconds, rho, own_factor=(a.cpu_factor == "own"))
            par = cb.pop("_parity", None)
            out["cpu_baseline"] = cb
            if par is not None:
                out["parity"] = par
        except Exception as exc:  # a host-side failure must not cost the measured GPU line
            out["cpu_baseline"] = {"value": None, "unit": "iterations/s", "cores": 1, "kind": "port", "error": repr(exc)}
    out.pop("_pmc_pair", None)


if __name__ == "__main__":
    main()
