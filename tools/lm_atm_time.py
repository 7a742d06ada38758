"""developer tool: time of one lm_atm step (off-grid bubble) by size, its split between the
multigrid solves and the kernels of csrc/lm_atm.hip, and the memory traffic of those kernels
against the time they take; `incompressible shear` in the same process for scale.

    python tools/lm_atm_time.py [nx ...]          (default: 128 1024 2048)

Per size: untimed steps until 50 ms of GPU work have passed, then >= 20 timed steps with a
device synchronise at the end; one more step under the per-kernel event profile
(Context.prof_report); the kernels' share is taken against the measured time per step.
Bytes per cell: the planes each kernel reads and writes once per cell (stencil neighbours
counted as cache hits), LM_TRAFFIC below, x launches per step."""
import contextlib
import io
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyro2_amd import device               # noqa: E402
from pyro2_amd.pyro_sim import Pyro        # noqa: E402

HBM = 8.0e12      # bytes / s, the MI355X figure the other tools compare with
OFFGRID = {"bubble.x_pert": 0.4037, "bubble.y_pert": 0.4519, "bubble.r_pert": 0.0913}
# doubles moved per cell and launch: planes read + planes written
LM_TRAFFIC = {"k_lm_coeff_src": 3, "k_lm_hat": 10, "k_lm_trans": 20, "k_lm_mac": 6,
              "k_lm_div_mac": 3, "k_lm_eta": 2, "k_lm_copy_b1": 2, "k_lm_mac_project": 6,
              "k_lm_rho_hat": 7, "k_lm_rho_int": 8, "k_lm_rho_trans": 13, "k_lm_rho_update": 7,
              "k_lm_eint_coeff": 4, "k_lm_vel_int": 14, "k_lm_advect": 14, "k_lm_buoy": 3,
              "k_lm_add_src": 3, "k_lm_div_cc": 5, "k_lm_proj_update": 10, "k_lm_dt_partial": 3}


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def timed(ctx, p, min_steps=20, warm_ms=50.0):
    gpu = 0.0
    while gpu < warm_ms:
        ctx.timer_start()
        quiet(p.single_step)
        gpu += ctx.timer_stop()
    ctx.sync()
    t0 = time.perf_counter()
    cyc = 0
    for _ in range(min_steps):
        quiet(p.single_step)
        cyc += sum(p.sim.mg_cycles)
    ctx.sync()
    ms = (time.perf_counter() - t0) / min_steps * 1e3
    ctx.prof_enable(True)
    quiet(p.single_step)
    prof = ctx.prof_report()
    ctx.prof_enable(False)
    return ms, cyc / min_steps, prof


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [128, 1024, 2048]
    ctx = device.Context(0)
    device.Context._default = ctx
    os.chdir(tempfile.mkdtemp())
    print("device:", ctx.info()["name"])
    for nx in sizes:
        over = {"mesh.nx": nx, "mesh.ny": nx, "driver.max_steps": 10**6, "driver.tmax": 1.e6}
        p = Pyro("lm_atm")
        quiet(p.initialize_problem, "bubble", inputs_dict=dict(OFFGRID, **over))
        ms, cyc, prof = timed(ctx, p)
        lm = {k: v for k, v in prof.items() if k.startswith("k_lm_")}
        t_lm = sum(t for _, t in lm.values())
        nbytes = sum(8.0 * LM_TRAFFIC.get(k, 0) * n for k, (n, _) in lm.items()) * nx * nx
        print(f"lm_atm bubble {nx}^2: {ms:.3f} ms per step, {cyc:.2f} V-cycles per step, "
              f"{ms / cyc:.3f} ms per V-cycle")
        # shares of the MEASURED step: the event profile does not see every launch (ghost fills,
        # the coefficient chain, the residual), so everything that is not a k_lm_* kernel --
        # the two solves, those launches, the gaps between launches -- is the remainder
        print(f"   lm_atm kernels {t_lm:.3f} ms = {100 * t_lm / ms:.1f} % of the step; multigrid "
              f"solves, coefficient chain, ghost fills, launch gaps {ms - t_lm:.3f} ms = "
              f"{100 * (ms - t_lm) / ms:.1f} %")
        print(f"   lm_atm kernels: {nbytes / (nx * nx):.0f} bytes per cell and step, "
              f"{nbytes / (t_lm * 1e-3) / 1e12:.2f} TB/s = {100 * nbytes / (t_lm * 1e-3) / HBM:.1f} % of 8 TB/s")
        for k, (n, t) in sorted(lm.items(), key=lambda kv: -kv[1][1])[:8]:
            bw = 8.0 * LM_TRAFFIC.get(k, 0) * n * nx * nx / (t * 1e-3) / 1e12
            print(f"      {k:20s} {n:3d} launches {t / n * 1e3:9.1f} us each  {bw:5.2f} TB/s")
        del p
        q = Pyro("incompressible")
        quiet(q.initialize_problem, "shear", inputs_dict=over)
        ms, cyc, _ = timed(ctx, q)
        print(f"incompressible shear {nx}^2: {ms:.3f} ms per step, {cyc:.2f} V-cycles per step, "
              f"{ms / cyc:.3f} ms per V-cycle")
        del q


if __name__ == "__main__":
    main()
