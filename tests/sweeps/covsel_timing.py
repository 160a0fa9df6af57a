"""Covariance selection: microseconds per iteration on the device, with the x-update (the eigen-step) split out, at
n = 64, 256, 1024 (m = 8n samples), next to the CPU restatement (the oracle loop with numpy's eigh on this host, one
BLAS thread, as bench.py labels its CPU leg).  Also the Jacobi sweeps per x-update: warm-started (the engine's way:
each x-update starts from the previous basis) and cold (a one-iteration run from the same iterates, whose only
x-update starts from V = I).  A checker-side measurement (imports the oracle), not part of the product.
    python tests/sweeps/covsel_timing.py [n ...]"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import admm_project_amd as ap  # noqa: E402
from covsel_restated import closures, cov, samples  # noqa: E402
from oracle import admm_ref  # noqa: E402

L = ap._lib
sizes = [int(a) for a in sys.argv[1:]] or [64, 256, 1024]
print("n | device us/iter | x-update us/iter | sweeps/x-update warm | cold | CPU oracle us/iter (1 BLAS thread)")
for n in sizes:
    D = samples(1, 8 * n, n)
    S = cov(D)
    lam, rho = 0.1, 1.0
    minx, minz, _ = ap.getproxops("covarianceselection", {"D": D, "lambda": lam})
    eng = minx.problem.engine
    K = 200 if n <= 256 else 40
    eng.run(rho=rho, maxiters=K, domaxiters=1, record_history=0)  # warm-up
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        eng.run(rho=rho, maxiters=K, domaxiters=1, record_history=0)
        best = min(best, time.perf_counter() - t0)
    warm = eng.info()["jacobi_sweeps"] / K
    eng.set_profiling([L.K_XSOLVE])
    eng.run(rho=rho, maxiters=K, domaxiters=1, record_history=0)
    xms, xcnt = eng.kernel_time(L.K_XSOLVE)
    eng.set_profiling(False)
    # cold sweeps: one-iteration runs from the iterates of a few points along the same run
    hist = eng.run(rho=rho, maxiters=K, domaxiters=1, record_history=1)
    X = eng.fetch(L.F_XVALS, n * n * K, (n * n, K))
    Z = eng.fetch(L.F_ZVALS, n * n * K, (n * n, K))
    U = eng.fetch(L.F_UVALS, n * n * K, (n * n, K))
    cold = []
    for k in (K // 4, K // 2, K - 1):
        eng.run(rho=rho, maxiters=1, domaxiters=1, record_history=0, x0=X[:, k], z0=Z[:, k], u0=U[:, k])
        cold.append(eng.info()["jacobi_sweeps"])
    # the CPU restatement: oracle loop, eigh, one BLAS thread
    xminf, zming, obj = closures(S, lam)
    Kc = 20 if n <= 256 else 3
    from threadpoolctl import threadpool_limits
    with threadpool_limits(limits=1, user_api="blas"):
        t0 = time.perf_counter()
        admm_ref.admm(xminf, zming, dict(A=1, B=-1, c=0, m=n * n, nA=n * n, nB=n * n, rho=rho, maxiters=Kc,
                                         domaxiters=1))
        cpu = (time.perf_counter() - t0) / Kc
    print(f"{n:5d} | {best / K * 1e6:10.1f} | {xms * 1e3 / max(xcnt, 1):10.1f} | {warm:6.2f} | "
          f"{np.mean(cold):6.2f} | {cpu * 1e6:10.1f}", flush=True)
    eng.close()
