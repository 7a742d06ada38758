"""developer tool: an ensemble of small Sedov runs stepped together against the same runs one after
the other (GPU box).

    python tools/ensemble_time.py [record.txt]        (profiles/ensemble_time.txt)

Sedov at 64^2, 128^2 and 256^2 (SIZES) in the contracted build, N = 1, 4, 16, 64 members (MEMBERS)
that differ in sedov.r_init, STEPS steps each: the wall time per step of the WHOLE ensemble through
Ensemble.run_sim() (pyrohip_comp_evolve_batch: two launches per step for all members) and, in the
same session, of the same N runs one after another through Pyro.run_sim() (pyrohip_comp_evolve:
two launches per step and member) -- what the code could do before.  Both include what a call pays
once: the members' first iteration (ghost fill + CFL reduction per member) and the read-back.
Pyro.run_sim() also runs its timers and sim.finalize() per member, which the ensemble pass does not:
host work of about a percent of 192 steps, in the ensemble's favour.
Warm-up: one untimed pass of both at every size (clocks, code objects, allocations), then REPS
repetitions, each on freshly initialised members (their set-up is not timed); median and spread
(max - min) are recorded.  Recorded, not a pass mark."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                    # noqa: E402

from pyro2_amd import device                                          # noqa: E402
from pyro2_amd.ensemble import Ensemble                               # noqa: E402
from pyro2_amd.pyro_sim import Pyro                                   # noqa: E402

SIZES = [int(x) for x in os.environ.get("SIZES", "64,128,256").split(",")]
MEMBERS = [int(x) for x in os.environ.get("MEMBERS", "1,4,16,64").split(",")]
REPS = int(os.environ.get("REPS", "3"))
STEPS = int(os.environ.get("STEPS", "192"))       # three batches of 64


def inputs(nx, m, n):
    return {"mesh.nx": nx, "mesh.ny": nx, "driver.max_steps": STEPS, "driver.tmax": 1.e30, "gpu.fast_math": 1,
            "sedov.r_init": 0.05 + 0.1 * m / max(n, 1), "io.do_io": 0, "vis.dovis": 0, "driver.verbose": 0}


def quiet(fn):
    """the members' parameter listings go nowhere"""
    out = sys.stdout
    sys.stdout = open(os.devnull, "w")
    try:
        return fn()
    finally:
        sys.stdout.close()
        sys.stdout = out


def ensemble_pass(ctx, nx, n):
    ens = Ensemble("compressible")
    quiet(lambda: [ens.add("sedov", "inputs.sedov", inputs(nx, m, n)) for m in range(n)])
    for p in ens.members:
        p.sim._device_state()         # (uploaded: not part of the stepping)
    ctx.sync()
    t0 = time.perf_counter()
    ens.run_sim()
    ctx.sync()
    dt = time.perf_counter() - t0
    assert all(p.sim.n == STEPS for p in ens.members)
    return 1e6 * dt / STEPS, [p.sim.cc_data.t for p in ens.members]


def sequential_pass(ctx, nx, n):
    runs = []
    for m in range(n):
        p = Pyro("compressible")
        quiet(lambda: p.initialize_problem("sedov", inputs_file="inputs.sedov", inputs_dict=inputs(nx, m, n)))
        p.sim._device_state()
        runs.append(p)
    ctx.sync()
    out = sys.stdout                  # (the runs' closing messages go nowhere: redirected once, outside the clock)
    sys.stdout = open(os.devnull, "w")
    try:
        t0 = time.perf_counter()
        for p in runs:
            p.run_sim()
        ctx.sync()
        dt = time.perf_counter() - t0
    finally:
        sys.stdout.close()
        sys.stdout = out
    assert all(p.sim.n == STEPS for p in runs)
    return 1e6 * dt / STEPS, [p.sim.cc_data.t for p in runs]


def main():
    rec = [a for a in sys.argv[1:] if not a.startswith("--")]
    ctx = device.Context.default()

    def say(line):
        print(line, flush=True)
        if rec:
            with open(rec[0], "a") as f:
                f.write(line + "\n")
    say(f"ensemble_time: Sedov, contracted build, {STEPS} steps per member; us per step of the WHOLE ensemble (wall, "
        f"synchronised at both ends); one warm-up pass, {REPS} repetitions: median (max - min)   "
        f"{time.strftime('%Y-%m-%d')}   {ctx.info()['name']}")
    say(f"{'grid':>7} {'N':>3}  {'ensemble':>22}  {'N runs in a row':>22}  {'ratio':>6}  {'ensemble / member':>17}")
    for nx in SIZES:            # warm-up: clocks, code objects, the context's scratch
        ensemble_pass(ctx, nx, 2)
        sequential_pass(ctx, nx, 2)
    for nx in SIZES:
        for n in MEMBERS:
            e, s = [], []
            for _ in range(REPS):
                a, ta = ensemble_pass(ctx, nx, n)
                b, tb = sequential_pass(ctx, nx, n)
                assert np.allclose(ta, tb, rtol=1e-9), (ta, tb)
                e.append(a)
                s.append(b)
            me, ms = float(np.median(e)), float(np.median(s))
            say(f"{nx:5d}^2 {n:3d}  {me:10.1f} ({max(e) - min(e):8.1f})  {ms:10.1f} ({max(s) - min(s):8.1f})  "
                f"{ms / me:6.2f}  {me / n:17.2f}")
    say("")


if __name__ == "__main__":
    main()
