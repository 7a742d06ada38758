"""developer tool: time per step of the advection_nonuniform kernel (slotted rotation, limiter 2,
contracted build, periodic) at 2048^2, 4096^2 and 8192^2 and, in the same session, of the uniform
kernel's one-launch-per-step path at the same sizes (GPU box).

    python tools/advnu_time.py            # SIZES=2048,4096,8192  FAST=1  LIM=2

Event timers around a batch of launches (one pyrohip_advnu_evolve call: no host work between
the steps), after at least 50 ms of untimed steps (README: the clocks ramp).  Prints, per size,
us per step, Gcell/s and the fraction of the 8 TB/s roofline at 32 B per cell update (a, u, v in,
a out); for the uniform kernel at its own 16 B per cell."""
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np                      # noqa: E402

from pyro2_amd import device            # noqa: E402

PEAK = 8.0e12      # B/s, HBM3E of the MI355X
SIZES = [int(s) for s in os.environ.get("SIZES", "2048,4096,8192").split(",")]
FAST = int(os.environ.get("FAST", "1"))
LIM = int(os.environ.get("LIM", "2"))
ctx = device.Context(0)
print("device:", ctx.info(), flush=True)


def timed(run, nsteps):
    """ms per step of run(n), which queues n steps; warm-up of >= 50 ms first"""
    ctx.timer_start()
    run(10)
    est = max(ctx.timer_stop() / 10.0, 1e-3)
    run(2 * int(np.ceil(25.0 / est)))                     # >= 50 ms, untimed
    ctx.sync()
    best, all_ms = None, []
    for _ in range(3):
        ctx.timer_start()
        run(nsteps)
        ms = ctx.timer_stop() / nsteps
        all_ms.append(ms)
        best = ms if best is None else min(best, ms)
    return best, all_ms


for nx in SIZES:
    x = (np.arange(nx + 8) + 0.5 - 4) / nx
    X, Y = np.meshgrid(x, x, indexing="ij")
    dens = ((X - 0.5)**2 + (Y - 0.75)**2 < 0.15**2).astype(np.float64)
    dens[(np.abs(X - 0.5) < 0.025) & (Y > 0.6) & (Y < 0.75)] = 0.0
    u, v = 0.5 * (Y - 0.5), -0.5 * (X - 0.5)
    dt = 0.8 * (1.0 / nx) / np.abs(u).max()
    nsteps = 200 if nx <= 2048 else (100 if nx <= 4096 else 40)
    per = ["periodic"] * 4
    st = device.DeviceState(ctx, nx, nx, 4, [per, per, per])
    st.upload(np.ascontiguousarray(np.stack([u, v, dens], axis=-1)))
    del X, Y
    ms, every = timed(lambda n: st.advnu_evolve(2, 0, 1, 1.0 / nx, 1.0 / nx, [dt] * n, LIM, fast_math=FAST), nsteps)
    cells = float(nx) * nx
    print(f"nonuniform nx={nx} fast={FAST} lim={LIM}: {1e3 * ms:9.2f} us/step  {cells / ms / 1e6:7.2f} Gcell/s  "
          f"{32 * cells / (ms * 1e-3) / PEAK:.3f} of 8 TB/s at 32 B/cell   (runs: "
          + " ".join(f"{1e3 * m:.2f}" for m in every) + ")", flush=True)
    out = st.download()[4:-4, 4:-4, 2]
    print(f"           density after the run: min {out.min():.6f} max {out.max():.6f} sum {out.sum():.6f}", flush=True)
    del st
    su = device.DeviceState(ctx, nx, nx, 4, [per])
    su.upload(np.ascontiguousarray(dens))

    def uniform(n):
        for _ in range(n):
            su.adv_step(0, 1.0 / nx, 1.0 / nx, 1.0, 1.0, 0.8 / nx, LIM, fill=True, fast_math=FAST)
    ms, every = timed(uniform, nsteps)
    print(f"uniform    nx={nx} fast={FAST} lim={LIM}: {1e3 * ms:9.2f} us/step  {cells / ms / 1e6:7.2f} Gcell/s  "
          f"{16 * cells / (ms * 1e-3) / PEAK:.3f} of 8 TB/s at 16 B/cell   (runs: "
          + " ".join(f"{1e3 * m:.2f}" for m in every) + ")", flush=True)
    del su
