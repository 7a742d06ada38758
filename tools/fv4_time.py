"""developer tool: what a step of compressible_fv4 / compressible_sdc costs (GPU box).

    PARENT=<checkout of the parent commit, built> python tools/fv4_time.py [record.txt]

Per step through Pyro.run_sim() (vis.dovis = 0, no output, gpu.fast_math = 1, CFL steps) of `acoustic_pulse`
at 64^2, 128^2, 256^2, 512^2 and 2048^2 (CASES: solver:n:steps per repetition), each in a child
process of its own under its own `timeout -k 10`, for this tree and for the tree at PARENT (a
commit whose can_evolve_many() answers no for these solvers takes the steps singly there).  The
first child that fails ends the tool: nothing more is started on the GPU behind it.  Per child: one
run_sim of WARM steps untimed, then REPS times "raise max_steps by the case's step count, run_sim,
synchronise", wall clock around each.  Prints ms per step of every repetition, the median, the
spread (max - min) and the ratio parent / this tree; a case in which this tree is slower than the
parent by more than the spread of the repetitions is flagged: can_evolve_many() should refuse that
regime.  The record belongs in profiles/fv4_evolve_time.txt.

    python tools/fv4_time.py --kernels

is the tool's earlier form: single steps at 1024^2 ... 4096^2 with the time of every kernel from the
library's HIP-event timers (kernel_times below; the numbers of DESIGN.md 3.x "Measured").

Only the public API is used."""
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

REPS = int(os.environ.get("REPS", "3"))
WARM = int(os.environ.get("WARM", "10"))
LIMIT = int(os.environ.get("CHILD_SECONDS", "240"))
CASES = [(s, int(n), int(c)) for s, n, c in (x.split(":") for x in os.environ.get(
    "CASES", "compressible_fv4:64:200,compressible_fv4:128:200,compressible_fv4:256:200,compressible_fv4:512:100,"
             "compressible_fv4:2048:10,compressible_sdc:64:100,compressible_sdc:128:100,compressible_sdc:256:100,"
             "compressible_sdc:512:50,compressible_sdc:2048:5").split(","))]


def run_sim_child(solver, n, steps):
    """one case in this process: prints "RS <ms per step> ... | <batched>" """
    p = Pyro(solver)
    p.initialize_problem("acoustic_pulse", inputs_file="inputs.acoustic_pulse", inputs_dict={
        "mesh.nx": n, "mesh.ny": n, "driver.max_steps": WARM, "driver.tmax": 1.0e9, "io.do_io": 0,
        "driver.verbose": 0, "vis.dovis": 0, "gpu.fast_math": 1,
        # (CFL steps: the problem's own fix_dt is chosen for 128^2 and breaks the 2048^2 run after five steps)
        "driver.fix_dt": -1.0})
    p._quiet = True
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


def _child(root, *args):
    env = dict(os.environ, PYRO_ROOT=root)
    out = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__)]
                         + [str(a) for a in args], env=env, capture_output=True, text=True)
    rows = [ln for ln in out.stdout.splitlines() if ln.startswith("RS ")]
    if out.returncode != 0 or not rows:
        sys.exit(f"child failed with status {out.returncode} ({root}, {args}); nothing more is started: "
                 f"{out.stdout[-2000:]} {out.stderr[-2000:]}")
    return rows[0]


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

    say(f"fv4_time: {WARM} warm-up steps + {REPS} repetitions per case; ms per step through Pyro.run_sim(), "
        "acoustic_pulse, gpu.fast_math = 1")
    say(f"commit {os.environ.get('COMMIT', '(this tree)')}   parent {os.environ.get('PARENT_COMMIT', parent)}   "
        f"{time.strftime('%Y-%m-%d')}   {device.Context.default().info()['name']}")
    trees = [("this tree", _HERE)] + ([("parent", parent)] if parent else [])
    for solver, n, steps in CASES:
        say(f"{solver} {n} x {n}, {steps} steps per repetition")
        res = {}
        for tag, root in trees:
            body, tail = _child(root, "--run-sim-child", solver, n, steps)[3:].split("|")
            res[tag] = [float(x) for x in body.split()]
            say(f"{tag:>12} ({'device loop' if int(tail) else 'single steps':>12}): " + _fmt(res[tag]))
        if len(res) == 2:
            a, b = res["this tree"], res["parent"]
            spread = max(max(a) - min(a), max(b) - min(b))
            slower = np.median(a) - np.median(b) > spread
            say(f"{'parent / this tree':>27}: {np.median(b) / np.median(a):9.2f}"
                + ("   SLOWER THAN THE PARENT BEYOND THE SPREAD" if slower else ""))
    say("")


def kernel_times():
    """--kernels: one compressible_fv4 RK4 step and one compressible_sdc step taken singly at 1024^2,
    2048^2, 4096^2, and compressible_rk RK4 at 4096^2 for comparison, in one process.  Each case is
    warmed up for >= 50 ms of steps first; the step time is the wall time of STEPS steps between two
    device synchronisations, the kernel times come from the library's HIP-event timers (pyrohip prof).
    SIZES="1024,2048,4096" STEPS=10 FAST=1."""
    import json
    import tempfile
    os.chdir(tempfile.mkdtemp())
    sizes = [int(s) for s in os.environ.get("SIZES", "1024,2048,4096").split(",")]
    steps = int(os.environ.get("STEPS", "10"))
    fast = int(os.environ.get("FAST", "1"))
    ctx = device.Context(0)
    device.Context._default = ctx

    def time_solver(solver, n):
        p = Pyro(solver)
        p.initialize_problem("acoustic_pulse", inputs_file="inputs.acoustic_pulse",
                             inputs_dict={"mesh.nx": n, "mesh.ny": n, "driver.fix_dt": 1.e-5,
                                          "driver.max_steps": 10**6, "driver.tmax": 1.e9,
                                          "gpu.fast_math": fast})
        t0 = time.perf_counter()
        while True:                     # warm-up: >= 50 ms and >= 2 steps
            p.single_step()
            ctx.sync()
            if time.perf_counter() - t0 >= 0.05 and p.sim.n >= 2:
                break
        ctx.prof_enable(True)
        t0 = time.perf_counter()
        for _ in range(steps):
            p.single_step()
        ctx.sync()
        t1 = time.perf_counter()
        prof = ctx.prof_report()
        ctx.prof_enable(False)
        kern = {k: {"calls": int(v[0]), "ms_per_call": float(v[1]) / max(int(v[0]), 1)} for k, v in prof.items()}
        return {"solver": solver, "n": n, "ms_per_step": 1e3 * (t1 - t0) / steps, "kernels": kern}

    out = []
    for n in sizes:
        for solver in ("compressible_fv4", "compressible_sdc"):
            out.append(time_solver(solver, n))
            print(json.dumps(out[-1]), flush=True)
    r = time_solver("compressible_rk", max(sizes))
    print(json.dumps(r), flush=True)
    fv4 = [x for x in out if x["solver"] == "compressible_fv4" and x["n"] == max(sizes)][0]
    print(f"fv4 / rk RK4 step at {max(sizes)}^2: {fv4['ms_per_step'] / r['ms_per_step']:.2f}x", flush=True)


if __name__ == "__main__":
    if "--run-sim-child" in sys.argv:
        k = sys.argv.index("--run-sim-child")
        run_sim_child(sys.argv[k + 1], *[int(x) for x in sys.argv[k + 2:k + 4]])
    elif "--kernels" in sys.argv:
        kernel_times()
    else:
        main()
