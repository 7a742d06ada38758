"""Generate tests/golden/comp_fv4_*.npz by RUNNING THE REFERENCE's compressible_fv4 /
compressible_sdc solvers (test infrastructure, build container only):

    cd /tmp && MPLBACKEND=Agg \\
      PYTHONPATH=<repo>/oracle/shim:<reference checkout> \\
      python3.9 <repo>/tools/gen_fv4_golden.py

The shim of oracle/ replaces numba.njit by the identity.  Nothing of the reference is copied:
its solvers are run and their inputs / outputs stored.
  comp_fv4_rhs.npz    right-hand sides (Simulation.substep) and fluxes of four states
  comp_fv4_runs.npz   a few RK4 steps of compressible_fv4 and SDC steps of compressible_sdc, 32^2
  comp_fv4_h5.npz     the stored acoustic_pulse_0160.h5 end states of both solvers
"""
import os
import sys
import tempfile

import h5py
import numpy as np

os.chdir(tempfile.mkdtemp())   # Pyro writes inputs.auto into cwd

import pyro.compressible_fv4.fluxes as flx   # noqa: E402
from pyro.pyro_sim import Pyro               # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
REF = os.path.dirname(os.path.abspath(sys.modules["pyro"].__file__))
NAMES = ["density", "energy", "x-momentum", "y-momentum"]


def save(name, **kw):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **kw)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def rhs_case(solver, problem, inputs, extra, steps):
    p = Pyro(solver)
    p.initialize_problem(problem, inputs_file=inputs, inputs_dict=dict(extra, **{"driver.verbose": 0}))
    for _ in range(steps):
        p.single_step()
    sim = p.sim
    sim.cc_data.fill_BC_all()
    if steps == 0:
        sim.dt = 1.e-3
    U = np.array(sim.cc_data.data)
    k = np.array(sim.substep(sim.cc_data))
    Fx, Fy = flx.fluxes(sim.cc_data, sim.rp, sim.ivars)
    bcs = [sim.cc_data.BCs[n] for n in NAMES]
    rows = np.array([[b.xlb, b.xrb, b.ylb, b.yrb] for b in bcs])
    g = sim.cc_data.grid
    rp = sim.rp
    meta = np.array([g.dx, g.dy, rp.get_param("eos.gamma"), rp.get_param("compressible.grav"),
                     rp.get_param("compressible.use_flattening"), rp.get_param("sponge.do_sponge"),
                     rp.get_param("sponge.sponge_rho_begin"), rp.get_param("sponge.sponge_rho_full"),
                     rp.get_param("sponge.sponge_timescale")])
    return dict(U=U, k=k, Fx=np.array(Fx), Fy=np.array(Fy), bcs=rows, meta=meta)


def gen_rhs():
    cases = {
        # the acoustic pulse initial condition at 32^2 (after preevolve)
        "pulse": ("compressible_fv4", "acoustic_pulse", "inputs.acoustic_pulse",
                  {"mesh.nx": 32, "mesh.ny": 32}, 0),
        # a shocked state on a 32 x 48 grid (square cells): flattening, limiter, viscosity
        "sod": ("compressible_fv4", "sod", "inputs.sod.y",
                {"mesh.nx": 32, "mesh.ny": 48, "mesh.xmax": 1.0 * 32 / 48, "driver.cfl": 0.5}, 6),
        # (compressible.use_flattening = 0 cannot be generated: fluxes.py:134-148 then blends
        # with the float 1.0 and fails on xi.v(); the device treats it as xi = 1)
        # gravity and the sponge, 24 x 40 (not a multiple of the tile)
        "rt": ("compressible_fv4", "rt", "inputs.rt",
               {"mesh.nx": 24, "mesh.ny": 40, "mesh.xmax": 0.5, "mesh.ymax": 0.5 * 40 / 24,
                "sponge.do_sponge": 1, "sponge.sponge_rho_begin": 1.5, "sponge.sponge_rho_full": 1.1},
               3),
    }
    out = {}
    for name, (solver, prob, inp, extra, steps) in cases.items():
        for key, v in rhs_case(solver, prob, inp, extra, steps).items():
            out[f"{name}_{key}"] = v
    out["cases"] = np.array(list(cases))
    save("comp_fv4_rhs", **out)


def gen_runs():
    out = {}
    for solver, steps in (("compressible_fv4", 4), ("compressible_sdc", 3)):
        p = Pyro(solver)
        p.initialize_problem("acoustic_pulse", inputs_file="inputs.acoustic_pulse",
                             inputs_dict={"mesh.nx": 32, "mesh.ny": 32, "driver.verbose": 0,
                                          "driver.fix_dt": -1.0, "driver.max_steps": steps})
        dts = []
        for _ in range(steps):
            p.single_step()
            dts.append(p.sim.dt)
        out[solver + "_dts"] = np.array(dts)
        out[solver + "_U"] = np.array(p.sim.cc_data.data)
        out[solver + "_t"] = np.array(p.sim.cc_data.t)
    save("comp_fv4_runs", **out)


def gen_h5():
    out = {}
    for solver in ("compressible_fv4", "compressible_sdc"):
        with h5py.File(f"{REF}/{solver}/tests/acoustic_pulse_0160.h5", "r") as f:
            out[solver + "_gold"] = np.stack([f["state/" + nm + "/data"][...] for nm in NAMES], axis=-1)
            out[solver + "_nsteps"] = np.array(int(f.attrs["nsteps"]))
            out[solver + "_time"] = np.array(float(f.attrs["time"]))
    save("comp_fv4_h5", **out)


if __name__ == "__main__":
    gen_h5()
    gen_rhs()
    gen_runs()
