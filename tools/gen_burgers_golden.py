"""Generate tests/golden/burgers_problems.npz by RUNNING THE REFERENCE's burgers solver on its
`tophat` and `converge` problems (test infrastructure, build container only):

    cd /tmp && MPLBACKEND=Agg \\
      PYTHONPATH=<repo>/oracle/shim:<reference checkout> \\
      python3 <repo>/tools/gen_burgers_golden.py

The shim of oracle/ replaces numba.njit by the identity.  Nothing of the reference is copied: its
solver is run and its inputs / outputs stored.

This checkout of the reference cannot start either problem as it stands: its
Pyro.initialize_problem reads the attribute PROBLEM_PARAMS of the problem module, and the two
modules do not define it.  The generator supplies `module.PROBLEM_PARAMS = {}` on the imported
module at run time (both problems have no parameters of their own: their _*.defaults files hold
an empty section); the reference's files are not touched.

Three runs, each by Pyro.single_step() (pyro_sim.py:241-281: fill_BC_all, compute_timestep,
evolve), prefix in the file:
  tophat_    `tophat` with its inputs.tophat: 32 x 32, periodic, limiter 2, 20 steps
  conv32_    `converge` with its inputs.converge.32 as shipped: 32 x 32, periodic, limiter 0,
             fix_dt = 0.01, 100 tracer particles on a grid, 12 steps
  conv2440_  `converge` with inputs.converge.32 on 24 x 40 cells, fix_dt = -1 (the CFL step of
             method_compute_timestep every step), limiter 1 and tmax = 2 (the CFL step is about 0.2:
             with the file's tmax = 1 the run would end after five), 100 tracer particles, 7 steps
Per run: `meta` (nx, ny, ng, dx, dy, limiter, cfl, fix_dt, n_particles or 0, tmax), `bc` (the four
sides), `ic` (u, v as initialised, (2, qx, qy)), `dts` (the dt of every step), `t` (the time
reached), `final` (u, v after the last step WITH their ghost frame: the boundary fill of the
state before that step), and with particles `part_pos` / `part_init` (positions and initial
positions in the set's order at the end).

The reference imports h5py at import time (util/io_pyro.py); without h5py a stub module stands
in for it.
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np

try:
    import h5py  # noqa: F401
except ImportError:
    sys.modules["h5py"] = types.ModuleType("h5py")

os.chdir(tempfile.mkdtemp())   # Pyro writes inputs.auto into cwd

from pyro.pyro_sim import Pyro                                # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")

RUNS = (
    ("tophat_", "tophat", "inputs.tophat", {}, 20),
    ("conv32_", "converge", "inputs.converge.32", {}, 12),
    ("conv2440_", "converge", "inputs.converge.32",
     {"mesh.nx": 24, "mesh.ny": 40, "driver.fix_dt": -1.0, "advection.limiter": 1, "driver.tmax": 2.0}, 7),
)


def planes(cc):
    return np.array([np.array(cc.get_var("x-velocity")), np.array(cc.get_var("y-velocity"))])


def run(problem, inputs, extra, nsteps):
    mod = importlib.import_module(f"pyro.burgers.problems.{problem}")
    if not hasattr(mod, "PROBLEM_PARAMS"):
        mod.PROBLEM_PARAMS = {}          # (what initialize_problem asks the module for)
    d = {"driver.verbose": 0, "io.do_io": 0, "vis.dovis": 0}
    d.update(extra)
    p = Pyro("burgers")
    p.initialize_problem(problem, inputs_file=inputs, inputs_dict=d)
    sim, rp = p.sim, p.rp
    g = sim.cc_data.grid
    out = {"ic": planes(sim.cc_data)}
    dts = []
    for _ in range(nsteps):
        assert not sim.finished()
        p.single_step()
        dts.append(float(sim.dt))
    npart = int(sim.particles.n_particles) if sim.particles is not None else 0
    out["meta"] = np.array([g.nx, g.ny, g.ng, g.dx, g.dy, rp.get_param("advection.limiter"),
                            rp.get_param("driver.cfl"), rp.get_param("driver.fix_dt"), npart,
                            rp.get_param("driver.tmax")], dtype=np.float64)
    out["bc"] = np.array([rp.get_param("mesh." + k) for k in ("xlboundary", "xrboundary", "ylboundary",
                                                              "yrboundary")])
    out["dts"] = np.array(dts)
    out["t"] = np.array(float(sim.cc_data.t))
    out["final"] = planes(sim.cc_data)
    if sim.particles is not None:
        out["part_pos"] = np.array(sim.particles.get_positions())
        out["part_init"] = np.array(sim.particles.get_init_positions())
    return out


def main():
    allout = {}
    for pre, problem, inputs, extra, nsteps in RUNS:
        for k, v in run(problem, inputs, extra, nsteps).items():
            allout[pre + k] = v
        print(pre, "dt[0], dt[-1] =", allout[pre + "dts"][0], allout[pre + "dts"][-1], " t =", allout[pre + "t"])
    path = os.path.join(OUT, "burgers_problems.npz")
    np.savez_compressed(path, **allout)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
