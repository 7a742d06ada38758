"""developer tool (GPU box): one compressible_fv4 RK4 step and one compressible_sdc step on the
acoustic pulse at 1024^2, 2048^2, 4096^2, and compressible_rk RK4 at 4096^2 for comparison, in
one process.  Each case is warmed up for >= 50 ms of steps first; the step time is the wall
time of STEPS steps between two device synchronisations, the kernel times come from the
library's HIP-event timers (pyrohip prof).  SIZES="1024,2048,4096" STEPS=10 FAST=1.
The kernel time per right-hand side: a separate run under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import tempfile
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
os.chdir(tempfile.mkdtemp())

from pyro2_amd import device              # noqa: E402
from pyro2_amd.pyro_sim import Pyro       # noqa: E402

SIZES = [int(s) for s in os.environ.get("SIZES", "1024,2048,4096").split(",")]
STEPS = int(os.environ.get("STEPS", "10"))
FAST = int(os.environ.get("FAST", "1"))
ctx = device.Context(0)
device.Context._default = ctx


def time_solver(solver, n):
    p = Pyro(solver)
    p.initialize_problem("acoustic_pulse", inputs_file="inputs.acoustic_pulse",
                         inputs_dict={"mesh.nx": n, "mesh.ny": n, "driver.fix_dt": 1.e-5,
                                      "driver.max_steps": 10**6, "driver.tmax": 1.e9,
                                      "gpu.fast_math": FAST})
    t0 = time.perf_counter()
    while True:                     # warm-up: >= 50 ms and >= 2 steps
        p.single_step()
        ctx.sync()
        if time.perf_counter() - t0 >= 0.05 and p.sim.n >= 2:
            break
    ctx.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(STEPS):
        p.single_step()
    ctx.sync()
    t1 = time.perf_counter()
    prof = ctx.prof_report()
    ctx.prof_enable(False)
    kern = {k: {"calls": int(v[0]), "ms_per_call": float(v[1]) / max(int(v[0]), 1)} for k, v in prof.items()}
    return {"solver": solver, "n": n, "ms_per_step": 1e3 * (t1 - t0) / STEPS, "kernels": kern}


out = []
for n in SIZES:
    for solver in ("compressible_fv4", "compressible_sdc"):
        r = time_solver(solver, n)
        out.append(r)
        print(json.dumps(r), flush=True)
r = time_solver("compressible_rk", max(SIZES))
out.append(r)
print(json.dumps(r), flush=True)
fv4 = [x for x in out if x["solver"] == "compressible_fv4" and x["n"] == max(SIZES)][0]
print(f"fv4 / rk RK4 step at {max(SIZES)}^2: {fv4['ms_per_step'] / r['ms_per_step']:.2f}x", flush=True)
