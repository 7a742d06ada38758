"""Read the HDF5 output files (layout of pyro/simulation_null.py:270-290 and
pyro/mesh/patch.py:750-788) back into a Simulation / CellCenterData2d, API of
pyro/util/io_pyro.py:27-148.  Files written by pyro itself are readable too
(same layout).  Host-side I/O through h5py, or through the pure-Python HDF5 code of
util/h5pure.py when h5py is not installed (util/h5lite.py picks)."""
import importlib

from ..mesh import boundary as bnd
from ..mesh.patch import Cartesian2d, CellCenterData2d, SphericalPolar


def _state_order(names, solver_name):
    """the variables of a file in the order the solver registered them, where that matters: a
    compressible state with passive scalars keeps density, energy and the momenta in front of
    them (compressible.Variables counts on it; the file lists its groups by name), the scalars in
    the order the solver names (compressible_react: fuel, ash), any other by name"""
    hydro = ["density", "energy", "x-momentum", "y-momentum"]
    if len(names) <= 4 or any(h not in names for h in hydro):
        return names
    if isinstance(solver_name, bytes):
        solver_name = solver_name.decode()
    known = [n for n in {"compressible_react": ["fuel", "ash"]}.get(solver_name, []) if n in names]
    return hydro + known + [n for n in names if n not in hydro + known]


def read(filename):
    from . import h5lite
    with h5lite.open_file(filename, "r") as f:
        solver_name = f.attrs.get("solver")
        problem_name = f.attrs.get("problem")
        t = f.attrs.get("time")
        nsteps = f.attrs.get("nsteps")
        g = f["grid"].attrs
        grid_class = SphericalPolar if g.get("coord_type", 0) == 1 else Cartesian2d   # io_pyro.py:52-60
        myg = grid_class(int(g["nx"]), int(g["ny"]), ng=int(g["ng"]), xmin=g["xmin"],
                         xmax=g["xmax"], ymin=g["ymin"], ymax=g["ymax"])
        names = _state_order(list(f["state"]), solver_name)
        dt, dt_old = f.attrs.get("dt"), f.attrs.get("dt_old")
        params = dict(f["runtime parameters"].attrs.items()) \
            if "runtime parameters" in f else {}
        # (cell averages of the fourth-order advection solver: its data class)
        if solver_name in ("advection_fv4", b"advection_fv4"):
            from ..mesh.fv import FV2d
            myd = FV2d(myg)
        else:
            myd = CellCenterData2d(myg)
        for n in names:
            a = f["state"][n].attrs
            known = {k: (a[k] if a[k] in bnd.bc_solid else "outflow")
                     for k in ("xlb", "xrb", "ylb", "yrb")}   # custom BC types: not filled here
            myd.register_var(n, bnd.BC(**known))
        myd.create()
        for k in f["aux"].attrs:
            myd.set_aux(k, f["aux"].attrs[k])
        for n in names:
            myd.get_var(n).v()[:, :] = f["state"][n]["data"][:, :]
        my_particles = None              # io_pyro.py:108-117
        if "particles" in f:
            from ..particles import particles
            pos = f["particles"]["particle_positions"][...]
            my_particles = particles.Particles(myd, None, len(pos), "array", pos,
                                               f["particles"]["init_particle_positions"][...])
    if solver_name is None:
        return myd
    if isinstance(solver_name, bytes):
        solver_name = solver_name.decode()
    base = {"compressible_rk": "compressible", "compressible_fv4": "compressible",
            "compressible_sdc": "compressible"}.get(solver_name, solver_name)
    try:
        solver = importlib.import_module("pyro2_amd." + base)
        sim = solver.Simulation(solver_name, problem_name, None, None)
    except ModuleNotFoundError:
        from ..simulation_null import NullSimulation
        sim = NullSimulation(solver_name, problem_name, None, None)
    sim.n = nsteps
    # what a restart needs beyond the state (Pyro.restart_problem)
    sim.restart_info = {"dt": dt, "dt_old": dt_old, "params": params}
    sim.cc_data = myd
    sim.particles = my_particles
    sim.cc_data.t = t
    # simulation-specific data (io_pyro.py:121: the base state of lm_atm)
    with h5lite.open_file(filename, "r") as f:
        sim.read_extras(f)
    try:
        derives = importlib.import_module(f"pyro2_amd.{base}.derives")
        sim.cc_data.add_derived(derives.derive_primitives)
    except ModuleNotFoundError:
        pass
    return sim
