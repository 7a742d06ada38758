"""developer tool: what a step of compressible_rk costs on small and middle grids (GPU box).

    PARENT=<checkout of the parent commit, built> python tools/comprk_time.py [record.txt]

Part 1, per step through Pyro.run_sim() (vis.dovis = 0, no output, CFL steps) of `sedov` with RK4 at
64^2, 128^2, 256^2, 512^2 and 1024^2 and with TVD2 at 256^2, in the contracted (gpu.fast_math = 1) and
the bit-faithful build (CASES: method:n:fast_math:steps per repetition), each in a child process of
its own under its own `timeout -k 10`, for this tree and for the tree at PARENT (a commit whose
can_evolve_many() answers no at these sizes takes the steps singly there, stage by stage).  The
first child that fails ends the tool: nothing more is started on the GPU behind it.  Per child: one
run_sim of WARM steps untimed, then REPS times "raise max_steps by the case's step count, run_sim,
synchronise", wall clock around each.  Prints ms per step of every repetition, the median, the
spread (max - min) and the ratio parent / this tree; a case in which this tree is slower than the
parent by more than the spread of the repetitions is flagged: the automatic kernel choice should
stay with the parent's path there.

Part 2, the step alone (pyrohip_comp_rk_step, RK4, Sedov) with gpu.kernel_set 1 (the stage tile
kernel) against 2 (the row-marching kernel) at 512^2, 1024^2, 1536^2 and 2048^2 (STEP_SIZES), both
builds, timed with the library's HIP events around STEP_N steps after STEP_WARM untimed ones, REPS
times, one child per size: the table the 2048^2 threshold of the automatic choice is read from.

The record belongs in profiles/comprk_tile_time.txt.  Only the public API is used."""
import os
import subprocess
import sys
import time

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_R = os.environ.get("PYRO_ROOT", _HERE)      # (the children: the tree whose package runs)
sys.path.insert(0, _R)
import numpy as np                      # noqa: E402

from pyro2_amd import device            # noqa: E402
from pyro2_amd.mesh import integration  # noqa: E402
from pyro2_amd.pyro_sim import Pyro     # noqa: E402

REPS = int(os.environ.get("REPS", "3"))
WARM = int(os.environ.get("WARM", "10"))
LIMIT = int(os.environ.get("CHILD_SECONDS", "240"))
CASES = [(m, int(n), int(f), int(c)) for m, n, f, c in (x.split(":") for x in os.environ.get(
    "CASES", "RK4:64:1:200,RK4:128:1:200,RK4:256:1:200,RK4:512:1:100,RK4:1024:1:40,TVD2:256:1:200,"
             "RK4:64:0:200,RK4:128:0:200,RK4:256:0:200,RK4:512:0:100,RK4:1024:0:40,TVD2:256:0:200").split(","))]
STEP_SIZES = [int(n) for n in os.environ.get("STEP_SIZES", "512,1024,1536,2048").split(",")]
STEP_N = int(os.environ.get("STEP_N", "20"))
STEP_WARM = int(os.environ.get("STEP_WARM", "5"))


def _sedov(method, n, fast, extra=None):
    p = Pyro("compressible_rk")
    p.initialize_problem("sedov", inputs_dict=dict({
        "mesh.nx": n, "mesh.ny": n, "driver.max_steps": WARM, "driver.tmax": 1.0e9, "io.do_io": 0,
        "driver.verbose": 0, "vis.dovis": 0, "gpu.fast_math": fast,
        "compressible.temporal_method": method}, **(extra or {})))
    p._quiet = True
    return p


def run_sim_child(method, n, fast, steps):
    """one case in this process: prints "RS <ms per step> ... | <batched>" """
    p = _sedov(method, n, fast)
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
    assert p.sim.n == WARM + REPS * steps
    refused = int(bool(getattr(p.sim, "_device_stepping_refused", False)))
    print("RS " + " ".join(f"{m:.6f}" for m in ms) + f" | {batched and not refused:d}", flush=True)


def step_child(n):
    """the step alone at n x n: prints "ST <kernel_set> <fast_math> <ms per step> ..." per combination"""
    a, b = integration.a["RK4"], integration.b["RK4"]
    ctx = device.Context.default()
    p = _sedov("RK4", n, 1)
    p.run_sim()                          # (WARM steps away from the initial point blast)
    ctx.sync()
    U0 = np.ascontiguousarray(np.array(p.sim.cc_data.data)[..., :4])
    g = p.sim.cc_data.grid
    dt = 0.5 * float(p.sim.dt)
    for fast in (1, 0):
        for ks in (1, 2):
            P = device.make_comp_params(g.dx, g.dy, fast_math=fast, kernel_set=ks)
            st = device.DeviceState(ctx, n, n, g.ng, [["outflow"] * 4] * 4)
            kst = device.DeviceState(ctx, n, n, g.ng, [["outflow"] * 4] * 16)
            st.upload(U0)
            assert st.comp_rk_can_fuse(P, kst, 4)
            for _ in range(STEP_WARM):
                st.comp_rk_step(P, kst, dt, a, b)
            ms = []
            for _ in range(REPS):
                ctx.sync()
                ctx.timer_start()
                for _ in range(STEP_N):
                    st.comp_rk_step(P, kst, dt, a, b)
                ms.append(ctx.timer_stop() / STEP_N)
            print(f"ST {ks} {fast} " + " ".join(f"{m:.6f}" for m in ms), flush=True)


def _child(root, *args):
    env = dict(os.environ, PYRO_ROOT=root)
    out = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__)]
                         + [str(a) for a in args], env=env, capture_output=True, text=True)
    rows = [ln for ln in out.stdout.splitlines() if ln.startswith(("RS ", "ST "))]
    if out.returncode != 0 or not rows:
        sys.exit(f"child failed with status {out.returncode} ({root}, {args}); nothing more is started: "
                 f"{out.stdout[-2000:]} {out.stderr[-2000:]}")
    return rows


def _fmt(ms):
    return (f"median {np.median(ms):9.4f} ms   spread {max(ms) - min(ms):7.4f}   runs "
            + " ".join(f"{m:.4f}" for m in ms))


def main():
    parent = os.environ.get("PARENT")
    if parent and not os.path.isdir(os.path.join(parent, "pyro2_amd")):
        sys.exit("PARENT must name a built checkout of the parent commit")
    rec = [a for a in sys.argv[1:] if not a.startswith("--")]

    def say(line):
        print(line, flush=True)
        if rec:
            with open(rec[0], "a") as f:
                f.write(line + "\n")

    say(f"comprk_time: {WARM} warm-up steps + {REPS} repetitions per case; ms per step through Pyro.run_sim(), "
        "compressible_rk sedov")
    say(f"commit {os.environ.get('COMMIT', '(this tree)')}   parent {os.environ.get('PARENT_COMMIT', parent)}   "
        f"{time.strftime('%Y-%m-%d')}   {device.Context.default().info()['name']}")
    trees = [("this tree", _HERE)] + ([("parent", parent)] if parent else [])
    if "--steps-only" not in sys.argv:
        for method, n, fast, steps in CASES:
            say(f"{method} {n} x {n}, gpu.fast_math = {fast}, {steps} steps per repetition")
            res = {}
            for tag, root in trees:
                body, tail = _child(root, "--run-sim-child", method, n, fast, steps)[0][3:].split("|")
                res[tag] = [float(x) for x in body.split()]
                say(f"{tag:>12} ({'device loop' if int(tail) else 'single steps':>12}): " + _fmt(res[tag]))
            if len(res) == 2:
                a, b = res["this tree"], res["parent"]
                spread = max(max(a) - min(a), max(b) - min(b))
                slower = np.median(a) - np.median(b) > spread
                say(f"{'parent / this tree':>27}: {np.median(b) / np.median(a):9.2f}"
                    + ("   SLOWER THAN THE PARENT BEYOND THE SPREAD" if slower else ""))
        say("")
    say(f"the step alone (pyrohip_comp_rk_step, RK4, sedov): HIP events around {STEP_N} steps, {REPS} repetitions; "
        "kernel_set 1 = stage tile kernel, 2 = row-marching kernel")
    for n in STEP_SIZES:
        med = {}
        for row in _child(_HERE, "--step-child", n):
            _, ks, fast, *ms = row.split()
            ms = [float(x) for x in ms]
            med[(int(ks), int(fast))] = float(np.median(ms))
            say(f"{n:5d} x {n:<5d} kernel_set {ks} fast_math {fast}: " + _fmt(ms))
        for fast in (1, 0):
            say(f"{n:5d} x {n:<5d} fast_math {fast}: row-marching / tile = {med[(2, fast)] / med[(1, fast)]:6.2f}")
    say("")


if __name__ == "__main__":
    if "--run-sim-child" in sys.argv:
        k = sys.argv.index("--run-sim-child")
        run_sim_child(sys.argv[k + 1], *[int(x) for x in sys.argv[k + 2:k + 5]])
    elif "--step-child" in sys.argv:
        step_child(int(sys.argv[sys.argv.index("--step-child") + 1]))
    else:
        main()
