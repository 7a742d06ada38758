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
path of a commit that has both).

    python tools/particles_time.py --run-sim [record.txt]      # PARENT=<checkout of the parent commit, built>

The second leg: what a particle run costs through Pyro.run_sim(), where the driver hands batches
of steps to the device (evolve_many) if the solver lets it.  compressible sedov at 64^2, 256^2 and
2048^2 (RS_SIZES) with NPART grid particles, each configuration in a child process of its own:
this tree with particles, the tree at PARENT with particles (a commit whose can_evolve_many
refuses a particle run steps singly there), this tree without particles.  Per child: one run_sim
of RS_WARM steps untimed, then REPS times "raise max_steps by the size's step count, run_sim,
synchronise", wall clock around each.  Prints ms per step of every repetition, medians, the ratio
parent / this tree and the increment over the particle-free run."""
import os
import subprocess
import sys
import time

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_R = os.environ.get("PYRO_ROOT", _HERE)      # (the --run-sim leg's children: the tree whose package runs)
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


# ---- the run_sim leg -------------------------------------------------------------------
RS_SIZES = [(int(a), int(b)) for a, b in (x.split(":") for x in
            os.environ.get("RS_SIZES", "64:2000,256:1000,2048:40").split(","))]   # nx:steps per repetition
RS_WARM = int(os.environ.get("RS_WARM", "30"))


def run_sim_child(nx, steps, npart):
    """one configuration in this process: prints "RS <ms per step> ... | <particles left> <batched>" """
    p = Pyro("compressible")
    d = {"mesh.nx": nx, "mesh.ny": nx, "driver.max_steps": RS_WARM, "driver.tmax": 1.0e9,
         "io.do_io": 0, "driver.verbose": 0, "vis.dovis": 0}
    if npart:
        d.update({"particles.do_particles": 1, "particles.n_particles": npart,
                  "particles.particle_generator": "grid"})
    p.initialize_problem("sedov", inputs_dict=d)
    p._quiet = True
    batched = int(bool(p.sim.can_evolve_many()))
    ctx = device.Context.default()
    p.run_sim()
    ctx.sync()
    ms = []
    for _ in range(REPS):
        p.sim.max_steps += steps
        t0 = time.perf_counter()
        p.run_sim()
        ctx.sync()
        ms.append(1e3 * (time.perf_counter() - t0) / steps)
    assert p.sim.n == RS_WARM + REPS * steps
    left = p.sim.particles.n_particles if npart else 0
    print("RS " + " ".join(f"{m:.6f}" for m in ms) + f" | {left} {batched}", flush=True)


def run_sim_leg():
    parent = os.environ.get("PARENT")
    if not parent or not os.path.isdir(os.path.join(parent, "pyro2_amd")):
        sys.exit("--run-sim: PARENT must name a built checkout of the parent commit")

    def child(root, nx, steps, npart):
        env = dict(os.environ, PYRO_ROOT=root)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--run-sim-child", str(nx), str(steps),
                              str(npart)], env=env, capture_output=True, text=True, timeout=900)
        row = [ln for ln in out.stdout.splitlines() if ln.startswith("RS ")]
        if out.returncode != 0 or not row:
            sys.exit(f"child failed ({root}, {nx}): {out.stdout[-2000:]} {out.stderr[-2000:]}")
        ms, tail = row[0][3:].split("|")
        left, batched = tail.split()
        return [float(x) for x in ms.split()], int(left), int(batched)

    lines = [f"particles_time --run-sim: compressible sedov through Pyro.run_sim, {NPART} grid particles, "
             f"{RS_WARM} warm-up steps + {REPS} repetitions",
             f"commit {os.environ.get('COMMIT', '(this tree)')}   parent {os.environ.get('PARENT_COMMIT', parent)}   "
             f"{time.strftime('%Y-%m-%d')}   {device.Context.default().info()['name']}"]
    for nx, steps in RS_SIZES:
        rows = {}
        for tag, root, npart in (("this tree, particles", _HERE, NPART), ("parent, particles", parent, NPART),
                                 ("this tree, none", _HERE, 0)):
            rows[tag] = child(root, nx, steps, npart)
        lines.append(f"{nx}^2, {steps} steps per repetition")
        for tag, (ms, left, batched) in rows.items():
            lines.append(f"{tag:>24} ({'device loop' if batched else 'single steps':>12}): median {np.median(ms):9.4f} ms/step   "
                         f"spread {max(ms) - min(ms):7.4f}   runs " + " ".join(f"{m:.4f}" for m in ms)
                         + (f"   ({left} particles left)" if "particles" in tag else ""))
        med = {k: float(np.median(v[0])) for k, v in rows.items()}
        lines.append(f"{'parent / this tree':>24}: {med['parent, particles'] / med['this tree, particles']:9.2f}")
        lines.append(f"{'particles - none':>24}: {1e3 * (med['this tree, particles'] - med['this tree, none']):9.1f} us/step")
    text = "\n".join(lines)
    print(text, flush=True)
    rec = [a for a in sys.argv[1:] if not a.startswith("--")]
    if rec:
        with open(rec[0], "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    if "--run-sim-child" in sys.argv:
        k = sys.argv.index("--run-sim-child")
        run_sim_child(*[int(x) for x in sys.argv[k + 1:k + 4]])
    elif "--run-sim" in sys.argv:
        run_sim_leg()
    else:
        main()
