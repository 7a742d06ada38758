"""developer tool: what a burgers step costs (GPU box).

    PARENT=<checkout of the parent commit, built> python tools/burgers_time.py [record.txt]

Leg 1, per step through Pyro.run_sim(): `test` (outflow) and `tophat` (periodic) at 64^2, 256^2,
2048^2 and 4096^2 (RS_SIZES), without and with NPART grid particles, each configuration in a child
process of its own, for this tree and for the tree at PARENT (a commit without the device-side
stepping loop takes the steps singly there; one without the problem reports n/a).  Per child: one
run_sim of RS_WARM steps untimed, then REPS times "raise max_steps by the size's step count,
run_sim, synchronise", wall clock around each.  Prints ms per step of every repetition, the
median, the spread (max - min) and the ratio parent / this tree.

Leg 2, the step alone: DeviceState.bg_step1 (k_bg_tile, one launch) against DeviceState.bg_step
(the four staged launches) at 2048^2 and 4096^2 (K_SIZES) on the `test` field: K_WARM calls
untimed, then REPS repetitions of K_CALLS calls, the kernels' own time from the library's event
timing (Context.prof_report) and the wall clock per call with a synchronisation at both ends.
A size at which the one-launch kernel is slower than the staged four by more than the spread is
flagged: evolve() should keep the staged kernels there.

Only the public API is used; what a tree lacks (bg_step1, can_evolve_many, a problem) is reported,
not an error."""
import os
import subprocess
import sys
import time

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_R = os.environ.get("PYRO_ROOT", _HERE)      # (the children: the tree whose package runs)
sys.path.insert(0, _R)
import numpy as np                      # noqa: E402

from pyro2_amd import device            # noqa: E402
from pyro2_amd.pyro_sim import Pyro     # noqa: E402

NPART = int(os.environ.get("NPART", "10000"))
REPS = int(os.environ.get("REPS", "3"))
RS_SIZES = [(int(a), int(b)) for a, b in (x.split(":") for x in
            os.environ.get("RS_SIZES", "64:2000,256:1000,2048:100,4096:40").split(","))]   # nx:steps per repetition
RS_WARM = int(os.environ.get("RS_WARM", "30"))
K_SIZES = [int(x) for x in os.environ.get("K_SIZES", "2048,4096").split(",")]
K_WARM = int(os.environ.get("K_WARM", "5"))
K_CALLS = int(os.environ.get("K_CALLS", "20"))
STAGED = ("k_bg_hat", "k_bg_trans", "k_bg_mac", "k_bg_update")


def _pyro(problem, nx, npart, max_steps):
    p = Pyro("burgers")
    d = {"mesh.nx": nx, "mesh.ny": nx, "driver.max_steps": max_steps, "driver.tmax": 1.0e9,
         "io.do_io": 0, "driver.verbose": 0, "vis.dovis": 0, "particles.do_particles": 0}
    if npart:
        d.update({"particles.do_particles": 1, "particles.n_particles": npart,
                  "particles.particle_generator": "grid"})
    p.initialize_problem(problem, inputs_dict=d)
    p._quiet = True
    return p


def run_sim_child(problem, nx, steps, npart):
    """one configuration in this process: prints "RS <ms per step> ... | <batched>" or "RS n/a" """
    try:
        p = _pyro(problem, nx, npart, RS_WARM)
    except Exception as e:                      # (a tree without the problem)
        print(f"RS n/a | {type(e).__name__}", flush=True)
        return
    probe = getattr(p.sim, "can_evolve_many", None)
    batched = int(bool(probe and probe()))
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
    print("RS " + " ".join(f"{m:.6f}" for m in ms) + f" | {batched}", flush=True)


def kernel_child(nx):
    """the step alone in this process: prints "KS <name> <kernel ms per call> ... | <wall ms per call> ..." """
    p = _pyro("test", nx, 0, 1)
    cc, g = p.sim.cc_data, p.sim.cc_data.grid
    cc.fill_BC_all()
    st = cc.device_state()
    ctx = st.ctx
    dt = 0.8 * g.dx / 3.0
    legs = [("staged", st.bg_step, STAGED)]
    if hasattr(st, "bg_step1"):
        legs.append(("one-launch", st.bg_step1, ("k_bg_tile",)))
    for name, step, kernels in legs:
        for _ in range(K_WARM):
            step(0, 1, g.dx, g.dy, dt, 2)
        ctx.sync()
        kms, wms = [], []
        for _ in range(REPS):
            ctx.prof_report()
            ctx.prof_enable(True)
            for _ in range(K_CALLS):
                step(0, 1, g.dx, g.dy, dt, 2)
            ctx.sync()
            rep = ctx.prof_report()
            ctx.prof_enable(False)
            kms.append(sum(rep[k][1] for k in kernels) / K_CALLS)
            t0 = time.perf_counter()
            for _ in range(K_CALLS):
                step(0, 1, g.dx, g.dy, dt, 2)
            ctx.sync()
            wms.append(1e3 * (time.perf_counter() - t0) / K_CALLS)
        print(f"KS {name} " + " ".join(f"{m:.6f}" for m in kms) + " | " + " ".join(f"{m:.6f}" for m in wms), flush=True)


def _child(root, *args):
    env = dict(os.environ, PYRO_ROOT=root)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], env=env,
                         capture_output=True, text=True, timeout=900)
    rows = [ln for ln in out.stdout.splitlines() if ln.startswith(("RS ", "KS "))]
    if out.returncode != 0 or not rows:
        sys.exit(f"child failed ({root}, {args}): {out.stdout[-2000:]} {out.stderr[-2000:]}")
    return rows


def _fmt(ms):
    return (f"median {np.median(ms):9.4f} ms   spread {max(ms) - min(ms):7.4f}   runs "
            + " ".join(f"{m:.4f}" for m in ms))


def main():
    parent = os.environ.get("PARENT")
    if parent and not os.path.isdir(os.path.join(parent, "pyro2_amd")):
        sys.exit("PARENT must name a built checkout of the parent commit")
    rec = [a for a in sys.argv[1:] if not a.startswith("--")]

    class Record(list):
        """the record's lines: printed, and appended to the file, as they come"""

        def append(self, line):
            super().append(line)
            print(line, flush=True)
            if rec:
                with open(rec[0], "a") as f:
                    f.write(line + "\n")

    lines = Record()
    for line in [f"burgers_time: {RS_WARM} warm-up steps + {REPS} repetitions per configuration; {NPART} grid particles",
             f"commit {os.environ.get('COMMIT', '(this tree)')}   parent {os.environ.get('PARENT_COMMIT', parent)}   "
             f"{time.strftime('%Y-%m-%d')}   {device.Context.default().info()['name']}",
             "leg 1: ms per step through Pyro.run_sim()"]:
        lines.append(line)
    trees = [("this tree", _HERE)] + ([("parent", parent)] if parent else [])
    for nx, steps in RS_SIZES:
        for problem in ("test", "tophat"):
            for npart in (0, NPART):
                lines.append(f"{problem} {nx}^2, {steps} steps per repetition, {npart} particles")
                med = {}
                for tag, root in trees:
                    row = _child(root, "--run-sim-child", problem, nx, steps, npart)[0]
                    body, tail = row[3:].split("|")
                    if body.strip() == "n/a":
                        lines.append(f"{tag:>12}: n/a ({tail.strip()}: the tree has no such problem)")
                        continue
                    ms = [float(x) for x in body.split()]
                    med[tag] = float(np.median(ms))
                    lines.append(f"{tag:>12} ({'device loop' if int(tail) else 'single steps':>12}): " + _fmt(ms))
                if len(med) == 2:
                    lines.append(f"{'parent / this tree':>27}: {med['parent'] / med['this tree']:9.2f}")
    lines.append(f"leg 2: the step alone on the `test` field, limiter 2, ms per call ({K_CALLS} calls per repetition)")
    for nx in K_SIZES:
        res = {}
        for row in _child(_HERE, "--kernel-child", nx):
            name, rest = row[3:].split(" ", 1)
            k, w = rest.split("|")
            res[name] = ([float(x) for x in k.split()], [float(x) for x in w.split()])
            lines.append(f"{nx}^2 {name:>10}: kernels " + _fmt(res[name][0]))
            lines.append(f"{'':>{len(str(nx)) + 13}}  wall    " + _fmt(res[name][1]))
        if len(res) == 2:
            a, b = res["staged"][0], res["one-launch"][0]
            spread = max(max(a) - min(a), max(b) - min(b))
            slower = np.median(b) - np.median(a) > spread
            lines.append(f"{nx}^2 staged / one-launch (kernels): {np.median(a) / np.median(b):6.2f}"
                         + ("   ONE-LAUNCH SLOWER THAN THE STAGED FOUR BEYOND THE SPREAD" if slower else ""))
            hbm_floor = 32.0 * nx * nx / 8.0e12 * 1e3     # 32 B per cell at 8 TB/s
            lines.append(f"{nx}^2 HBM floor of 32 B/cell at 8 TB/s: {hbm_floor:.4f} ms")
    lines.append("")


if __name__ == "__main__":
    if "--run-sim-child" in sys.argv:
        k = sys.argv.index("--run-sim-child")
        run_sim_child(sys.argv[k + 1], *[int(x) for x in sys.argv[k + 2:k + 5]])
    elif "--kernel-child" in sys.argv:
        kernel_child(int(sys.argv[sys.argv.index("--kernel-child") + 1]))
    else:
        main()
