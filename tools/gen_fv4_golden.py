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
  comp_fv4_edges.npz  right-hand sides at ragged and sub-tile grids, dx != dy, heating, quad,
                      a density floor with ghosts below it
  comp_fv4_edge_runs.npz  compressible_fv4 / compressible_sdc steps on ragged non-periodic grids

    python3 gen_fv4_golden.py [h5] [rhs] [runs] [edges]     (default: all four)

The reference imports h5py at import time (util/io_pyro.py); without h5py a stub module
stands in for it and the h5 fixture is skipped.
"""
import os
import sys
import tempfile
import types

import numpy as np

try:
    import h5py
except ImportError:
    h5py = None
    sys.modules["h5py"] = types.ModuleType("h5py")

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


def rhs_case(solver, problem, inputs, extra, steps, keep_centres=False, out_state=False):
    p = Pyro(solver)
    if keep_centres:
        # non-square cells: preevolve asserts dx == dy, substep does not need it
        sim_cls = sys.modules["pyro.compressible_fv4.simulation"].Simulation
        pre = sim_cls.preevolve
        sim_cls.preevolve = lambda self: None
    try:
        p.initialize_problem(problem, inputs_file=inputs, inputs_dict=dict(extra, **{"driver.verbose": 0}))
    finally:
        if keep_centres:
            sim_cls.preevolve = pre
    for _ in range(steps):
        p.single_step()
    sim = p.sim
    sim.cc_data.fill_BC_all()
    if steps == 0:
        sim.dt = 1.e-3
    U = np.array(sim.cc_data.data)
    k = np.array(sim.substep(sim.cc_data))
    Uout = np.array(sim.cc_data.data)
    Fx, Fy = flx.fluxes(sim.cc_data, sim.rp, sim.ivars)
    bcs = [sim.cc_data.BCs[n] for n in NAMES]
    rows = np.array([[b.xlb, b.xrb, b.ylb, b.yrb] for b in bcs])
    g = sim.cc_data.grid
    rp = sim.rp
    meta = np.array([g.dx, g.dy, rp.get_param("eos.gamma"), rp.get_param("compressible.grav"),
                     rp.get_param("compressible.use_flattening"), rp.get_param("sponge.do_sponge"),
                     rp.get_param("sponge.sponge_rho_begin"), rp.get_param("sponge.sponge_rho_full"),
                     rp.get_param("sponge.sponge_timescale")])
    out = dict(U=U, k=k, Fx=np.array(Fx), Fy=np.array(Fy), bcs=rows, meta=meta)
    if out_state:
        out["Uout"] = Uout
        out["small_dens"] = np.array(rp.get_param("compressible.small_dens"))
    if sim.problem_source is not None:
        # heating.py source_terms: S[E] = rho e_rate exp(-(dist / r_src)**2)
        xc, yc = 0.5 * (g.xmin + g.xmax), 0.5 * (g.ymin + g.ymax)
        dist = np.sqrt((g.x2d - xc)**2 + (g.y2d - yc)**2)
        out["heat"] = np.exp(-(dist / rp.get_param("heating.r_src"))**2)
        out["heat_rate"] = np.array(rp.get_param("heating.e_rate"))
    return out


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


def run_case(solver, problem, inputs, extra, steps, pre=""):
    p = Pyro(solver)
    p.initialize_problem(problem, inputs_file=inputs,
                         inputs_dict=dict(extra, **{"driver.verbose": 0, "driver.fix_dt": -1.0,
                                                    "driver.max_steps": steps}))
    dts = []
    for _ in range(steps):
        p.single_step()
        dts.append(p.sim.dt)
    return {pre + solver + "_dts": np.array(dts), pre + solver + "_U": np.array(p.sim.cc_data.data),
            pre + solver + "_t": np.array(p.sim.cc_data.t)}


def gen_runs():
    out = {}
    for solver, steps in (("compressible_fv4", 4), ("compressible_sdc", 3)):
        out.update(run_case(solver, "acoustic_pulse", "inputs.acoustic_pulse", {"mesh.nx": 32, "mesh.ny": 32},
                            steps))
    save("comp_fv4_runs", **out)


# ragged tiles (8 x 32 cells, x rows by y columns), grids below one tile, dx != dy, heating
EDGE_RHS = {
    # 21 x 13: ragged both ways, below one tile in y; outflow x, reflect y.  small_dens sits
    # above the right state's density: clean_state floors the interior only, the outflow
    # ghosts keep the lower density
    "sodx": ("compressible_fv4", "sod", "inputs.sod.x",
             {"mesh.nx": 21, "mesh.ny": 13, "mesh.xmax": 1.0, "mesh.ymax": 13 / 21,
              "driver.cfl": 0.5, "compressible.small_dens": 0.13}, 3, False),
    # 13 x 70: ragged x below one tile, three y tiles with a ragged last one; hse boundaries,
    # gravity and the sponge
    "rt": ("compressible_fv4", "rt", "inputs.rt",
           {"mesh.nx": 13, "mesh.ny": 70, "mesh.xmax": 0.5, "mesh.ymax": 0.5 * 70 / 13,
            "sponge.do_sponge": 1, "sponge.sponge_rho_begin": 1.5, "sponge.sponge_rho_full": 1.1}, 3, False),
    # the heating profile (problem source) on the unmasked centres; a strong source, so that
    # after three steps every variable's k carries the flow it drives (at e_rate = 0.1 the gas
    # is still at rest and k of the density and momenta is ~1e-6 of the flux terms)
    "heating": ("compressible_fv4", "heating", "inputs.heating",
                {"mesh.nx": 18, "mesh.ny": 18, "heating.e_rate": 1000.0}, 3, False),
    # four states: strong discontinuities and shear, limiter branches, artificial viscosity
    "quad": ("compressible_fv4", "quad", "inputs.quad", {"mesh.nx": 20, "mesh.ny": 20}, 3, False),
    # dy = 1.5 dx: the cell-centre pulse without preevolve (which asserts square cells)
    "pulse_dy": ("compressible_fv4", "acoustic_pulse", "inputs.acoustic_pulse",
                 {"mesh.nx": 16, "mesh.ny": 16, "mesh.ymax": 1.5}, 0, True),
}


def gen_edges():
    out = {}
    for name, (solver, prob, inp, extra, steps, centres) in EDGE_RHS.items():
        for key, v in rhs_case(solver, prob, inp, extra, steps, keep_centres=centres, out_state=True).items():
            out[f"{name}_{key}"] = v
    out["cases"] = np.array(list(EDGE_RHS))
    save("comp_fv4_edges", **out)
    runs = {}
    grids = {"sodx": ("sod", "inputs.sod.x", {"mesh.nx": 44, "mesh.ny": 12, "mesh.xmax": 1.0,
                                               "mesh.ymax": 12 / 44}),
             "rt": ("rt", "inputs.rt", {"mesh.nx": 12, "mesh.ny": 36, "mesh.xmax": 0.5, "mesh.ymax": 1.5})}
    for name, (prob, inp, extra) in grids.items():
        for solver, steps in (("compressible_fv4", 4), ("compressible_sdc", 3)):
            runs.update(run_case(solver, prob, inp, extra, steps, pre=name + "_"))
    runs["grids"] = np.array(list(grids))
    save("comp_fv4_edge_runs", **runs)


def gen_h5():
    out = {}
    for solver in ("compressible_fv4", "compressible_sdc"):
        with h5py.File(f"{REF}/{solver}/tests/acoustic_pulse_0160.h5", "r") as f:
            out[solver + "_gold"] = np.stack([f["state/" + nm + "/data"][...] for nm in NAMES], axis=-1)
            out[solver + "_nsteps"] = np.array(int(f.attrs["nsteps"]))
            out[solver + "_time"] = np.array(float(f.attrs["time"]))
    save("comp_fv4_h5", **out)


if __name__ == "__main__":
    what = sys.argv[1:] or ["h5", "rhs", "runs", "edges"]
    if "h5" in what:
        if h5py is None:
            print("h5py missing: comp_fv4_h5.npz not written")
        else:
            gen_h5()
    if "rhs" in what:
        gen_rhs()
    if "runs" in what:
        gen_runs()
    if "edges" in what:
        gen_edges()
