"""developer tool: time per Runge-Kutta step of advection_rk, advection_fv4 (the solvers' default
limiters) and advection_weno (weno_order 3 and 2) -- RK4, periodic -- at 2048^2 and 4096^2, both
builds, and in the same process of the
stage-by-stage path (pyrohip_state_lincomb + ghost fill + pyrohip_advrk_rhs per stage, the final
pyrohip_state_lincomb) that the fused step replaces (GPU box).

    python tools/advrk_time.py [out.json]        # SIZES=2048,4096 SCHEMES=2,4,5

Event timers around a batch of steps (one pyrohip_advrk_evolve call: no host work between the
steps), after at least 50 ms of untimed steps (the clocks ramp); best of three batches, all three
printed.  Beside each figure: the HBM floor of the step -- per stage one read of the state, s reads
of earlier increments and one write (the last stage writes the new state instead of its
increment), 8 B per cell each, over 8 TB/s -- and, as context, the one-launch CTU step of the
advection solver at 2048^2 (21.3 us, README)."""
import json
import os
import subprocess
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np                      # noqa: E402

from pyro2_amd import _lib, device      # noqa: E402
from pyro2_amd.mesh import integration  # noqa: E402

PEAK = 8.0e12      # B/s, HBM3E of the MI355X
SIZES = [int(s) for s in os.environ.get("SIZES", "2048,4096").split(",")]
SCHEMES = [int(s) for s in os.environ.get("SCHEMES", "2,4,5").split(",")]
# (scheme, limiter, weno_order)
CONFIGS = [c for c in ((2, 2, 0), (4, 1, 0), (5, 0, 3), (5, 0, 2)) if c[0] in SCHEMES]
METHOD = "RK4"
CTU_2048_US = 21.3
ctx = device.Context(0)
print("device:", ctx.info(), flush=True)


def timed(run, nsteps):
    """ms per step of run(n), which queues n steps; warm-up of >= 50 ms first, timed windows of
    at least nsteps steps and 200 ms"""
    ctx.timer_start()
    run(5)
    est = max(ctx.timer_stop() / 5.0, 1e-3)
    run(2 * int(np.ceil(25.0 / est)))                     # >= 50 ms, untimed
    ctx.sync()
    n = max(nsteps, int(np.ceil(200.0 / est)))
    all_ms = []
    for _ in range(3):
        ctx.timer_start()
        run(n)
        all_ms.append(ctx.timer_stop() / n)
    return min(all_ms), all_ms


def floor_us(cells, ns):
    """stage s reads y and s increments and writes one plane"""
    planes = sum(1 + s + 1 for s in range(ns))
    return 8.0 * planes * cells / PEAK * 1e6


results = []
for nx in SIZES:
    x = (np.arange(nx + 8) + 0.5 - 4) / nx
    X, Y = np.meshgrid(x, x, indexing="ij")
    dens = 1.0 + np.exp(-60.0 * ((X - 0.5)**2 + (Y - 0.5)**2))
    del X, Y
    dx = 1.0 / nx
    dt = 0.8 / (1.0 / dx + 1.0 / dx)
    nsteps = 100 if nx <= 2048 else 30
    per = [["periodic"] * 4]
    cells = float(nx) * nx
    ns = len(integration.b[METHOD])
    for scheme, lim, order in CONFIGS:
        for fast in (1, 0):
            P = _lib.AdvRkParams(dx, dx, 1.0, 1.0, lim, scheme, fast)
            P.weno_order, P.alpha = order, float(np.sqrt(1.0**2 + 1.0**2))
            st = device.DeviceState(ctx, nx, nx, 4, per)
            st.upload(np.ascontiguousarray(dens[:, :, None]))
            ms, every = timed(lambda n: st.advrk_evolve(0, P, METHOD, [dt] * n), nsteps)
            out = st.download()[4:-4, 4:-4, 0]
            del st
            su = device.DeviceState(ctx, nx, nx, 4, per)
            su.upload(np.ascontiguousarray(dens[:, :, None]))
            rk = integration.RKIntegrator(0.0, dt, method=METHOD)
            rk.set_start(su)

            def unfused(n):
                for _ in range(n):
                    for s in range(ns):
                        y = rk.get_stage_start(s)
                        y.fill_bc(-1)
                        y.advrk_rhs(0, P, rk.k, s)
                    rk.compute_final_update()
            ums, uevery = timed(unfused, max(nsteps // 2, 5))
            del su, rk
            rec = {"nx": nx, "scheme": scheme, "limiter": lim, "weno_order": order, "fast_math": fast,
                   "method": METHOD,
                   "us_per_step": 1e3 * ms, "runs_us": [1e3 * m for m in every],
                   "unfused_us_per_step": 1e3 * ums, "unfused_runs_us": [1e3 * m for m in uevery],
                   "hbm_floor_us": floor_us(cells, ns), "gcell_per_s": cells / ms / 1e6,
                   "ctu_advection_2048_us": CTU_2048_US,
                   "density_min_max_sum": [float(out.min()), float(out.max()), float(out.sum())]}
            results.append(rec)
            print(f"scheme {scheme} lim {lim} order {order} nx={nx} fast={fast}: {1e3 * ms:9.2f} us/step "
                  f"({cells / ms / 1e6:6.2f} Gcell/s; floor {rec['hbm_floor_us']:.1f} us = "
                  f"{rec['hbm_floor_us'] / (1e3 * ms):.2f} of it)   stage by stage {1e3 * ums:9.2f} us/step "
                  f"(x{ums / ms:.2f})   runs: " + " ".join(f"{1e3 * m:.1f}" for m in every)
                  + " | " + " ".join(f"{1e3 * m:.1f}" for m in uevery), flush=True)

if len(sys.argv) > 1:
    try:
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=_R, capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    with open(sys.argv[1], "w") as f:
        json.dump({"tool": "tools/advrk_time.py", "device": str(ctx.info()), "date": time.strftime("%Y-%m-%d"),
                   "commit": commit or "working tree", "results": results}, f, indent=1)
    print("wrote", sys.argv[1])
