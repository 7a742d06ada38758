"""developer tool: what tracer particles add to a time step (GPU box).

    python tools/particles_time.py [record.txt]      # NX=2048  NPART=10000  STEPS=20  WARM=5  REPS=3

`compressible` sedov at NX^2 through Pyro.single_step -- boundary fill, time step, evolve, the
tracers' update --, once without particles and once with NPART grid particles: WARM untimed steps,
then REPS repetitions of STEPS steps each, wall clock around the steps with a device
synchronisation at both ends (the host's share of a step is part of what is measured).  Prints
the ms per step of every repetition, the median of each run, the spread (max - min over the
repetitions) and the difference "with particles - without".

Only the public API is used, so the same script runs on a commit from before the device path
(there the tracers' velocity is derived on the host from a download of the whole state);
gpu.device_particles is set only where the parameter exists (DEVICE_PARTICLES=0 times the host
path of a commit that has both)."""
import os
import subprocess
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np                      # noqa: E402

from pyro2_amd import device            # noqa: E402
from pyro2_amd.pyro_sim import Pyro     # noqa: E402

NX = int(os.environ.get("NX", "2048"))
NPART = int(os.environ.get("NPART", "10000"))
STEPS = int(os.environ.get("STEPS", "20"))
WARM = int(os.environ.get("WARM", "5"))
REPS = int(os.environ.get("REPS", "3"))
DEVP = int(os.environ.get("DEVICE_PARTICLES", "1"))


def run(npart):
    """ms per step of the REPS repetitions"""
    p = Pyro("compressible")
    d = {"mesh.nx": NX, "mesh.ny": NX, "driver.max_steps": WARM + REPS * STEPS + 1, "driver.tmax": 1.0e9,
         "io.do_io": 0, "driver.verbose": 0, "vis.dovis": 0}
    mode = "none"
    if npart:
        d.update({"particles.do_particles": 1, "particles.n_particles": npart,
                  "particles.particle_generator": "grid"})
        try:
            p.rp.get_param("gpu.device_particles")
            d["gpu.device_particles"] = DEVP
            mode = "device" if DEVP else "host"
        except (KeyError, RuntimeError):
            mode = "host"               # (a commit from before the device path)
    p.initialize_problem("sedov", inputs_dict=d)
    ctx = device.Context.default()
    for _ in range(WARM):
        p.single_step()
    ctx.sync()
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(STEPS):
            p.single_step()
        ctx.sync()
        ms.append(1e3 * (time.perf_counter() - t0) / STEPS)
    n = p.sim.particles.n_particles if npart else 0
    return ms, mode, n


def main():
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=_R, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    commit = os.environ.get("COMMIT", commit)
    lines = [f"particles_time: compressible sedov {NX}^2, Pyro.single_step, {WARM} warm-up + {REPS} x {STEPS} steps",
             f"commit {commit}   {time.strftime('%Y-%m-%d')}   {device.Context.default().info()['name']}"]
    res = {}
    for tag, npart in (("without particles", 0), (f"with {NPART} particles", NPART)):
        ms, mode, n = run(npart)
        res[tag] = ms
        lines.append(f"{tag:>24} ({'tracers: ' + mode:>15}): median {np.median(ms):9.3f} ms/step   "
                     f"spread {max(ms) - min(ms):7.3f}   runs " + " ".join(f"{m:.3f}" for m in ms)
                     + (f"   ({n} particles left)" if npart else ""))
    a, b = (np.median(v) for v in res.values())
    lines.append(f"{'with - without':>24}: {b - a:9.3f} ms/step")
    text = "\n".join(lines)
    print(text, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
