"""Generate tests/golden/comp_scalars.npz by RUNNING THE REFERENCE's compressible solver with
passive scalars (test infrastructure, build container only):

    cd /tmp && MPLBACKEND=Agg \\
      PYTHONPATH=<repo>/oracle/shim:<reference checkout> \\
      python3 <repo>/tools/gen_comp_scalars_golden.py

The shim of oracle/ replaces numba.njit by the identity.  Nothing of the reference is copied: its
solver is run and its inputs / outputs stored.

The reference's characteristic tracing (compressible/interface.py, states()) assigns the four
hydro eigenvalues to the WHOLE eigenvalue vector, whose length is nvar: with scalars the
assignment fails.  The same routine of its swe solver writes the slice [:ns].  This tool reads the
source of pyro.compressible.interface at run time, gives the two assignments that slice IN MEMORY
(asserting that it found exactly two) and executes the result in the module's namespace.  No
other line changes, and the scalar-free runs below go through the untouched routine.

`compressible` is run through a subclass that passes extra_vars (compressible_react's _defaults
lack keys the solver reads).

Cases c<k>_ (3 steps each under the driver's dt policy):
  meta, bc, riemann     as in comp_rk.npz (oracle/gen_golden.py)
  ic                    the initial state with its unfilled ghost frame: density, energy,
                        x-momentum, y-momentum, fuel, ash
  dts, final            the dt of every step, the state after the last
  f1_final  (c0-c2)     the same run with fuel alone (5 variables)
  h_final   (c0-c2)     the 6-variable run with the initial fuel plane halved
Hydro state: rho, E = 1 + U(-0.3, 0.3) (E + 2), momenta U(-0.3, 0.3), seeded per case; c1 and c3
carry an energy jump of 10^3 across a tile seam of the 14 x 30 tile kernel (c1: one tile -- the
jump sits in its middle).  Scalars: fuel = rho U(0, 1), ash = rho - fuel.

Nothing is written unless, on the reference's own runs,
  (a) hydro planes and dts of every scalar run are np.array_equal to the unpatched 4-variable run
  (b) halving the fuel halves its plane exactly
  (c) the fuel plane is the same with and without ash
  (d) the file stays under 1 MB.

react_flame_ic / react_rt_ic: the initial data of compressible_react's problems flame (32 x 32)
and rt (16 x 48) as their init_data leaves them (6 variables).
"""
import importlib
import inspect
import os
import shutil
import sys
import tempfile
import types

import numpy as np

try:
    import h5py  # noqa: F401
except ImportError:
    sys.modules["h5py"] = types.ModuleType("h5py")

os.chdir(tempfile.mkdtemp())   # Pyro writes inputs.auto into cwd

import pyro.compressible.interface as ifc                     # noqa: E402
from pyro import compressible                                 # noqa: E402
from pyro.pyro_sim import Pyro                                # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
SIDES = ("mesh.xlboundary", "mesh.xrboundary", "mesh.ylboundary", "mesh.yrboundary")
NSTEPS = 3


def sides(xl, xr, yl, yr):
    return dict(zip(SIDES, (xl, xr, yl, yr)))


# (nx, ny, sides, Riemann solver, limiter, extra parameters, (i, j) of the energy jump or None)
CASES = [
    (4, 4, sides(*["periodic"] * 4), "HLLC", 2, {}, None),
    (14, 30, sides(*["outflow"] * 4), "HLLC", 2, {}, (7, 15)),
    (15, 31, sides(*["reflect"] * 4), "HLLC", 1, {}, None),
    (29, 61, sides("outflow", "outflow", "periodic", "periodic"), "HLLC_lm", 2,
     {"compressible.grav": -1.0}, (14, 30)),
    (31, 13, sides("reflect", "reflect", "periodic", "periodic"), "HLLC", 0,
     {"compressible.use_flattening": 0}, None),
]
PROPERTY_CASES = (0, 1, 2)

ORIGINAL_STATES = ifc.states


def patched_states():
    """states() of pyro.compressible.interface with the eigenvalue assignments on [:ns]"""
    src = inspect.getsource(ifc)
    old = "e_val[:] = np.array("
    assert src.count(old) == 2, src.count(old)
    ns = dict(ifc.__dict__)
    exec(compile(src.replace(old, "e_val[:ns] = np.array("), ifc.__file__, "exec"), ns)
    return ns["states"]


PATCHED_STATES = patched_states()


def scalar_sim(extra):
    class Sim(compressible.Simulation):
        def initialize(self):       # pylint: disable=arguments-differ
            super().initialize(extra_vars=list(extra))
    return Sim


def rough(seed, jump, fuel_scale):
    def init(my_data, rp):
        g = my_data.grid
        rng = np.random.default_rng(seed)
        r = rng.random((5, g.qx, g.qy))
        rho = 1.0 + 0.3 * (2.0 * r[0] - 1.0)
        ener = 3.0 + 0.3 * (2.0 * r[1] - 1.0)
        if jump is not None:
            ener[g.ng + jump[0]:, g.ng + jump[1]:] *= 1.e3
        my_data.get_var("density")[:, :] = rho
        my_data.get_var("energy")[:, :] = ener
        my_data.get_var("x-momentum")[:, :] = 0.3 * (2.0 * r[2] - 1.0)
        my_data.get_var("y-momentum")[:, :] = 0.3 * (2.0 * r[3] - 1.0)
        fuel = rho * r[4]
        if "fuel" in my_data.names:
            my_data.get_var("fuel")[:, :] = fuel_scale * fuel
        if "ash" in my_data.names:
            my_data.get_var("ash")[:, :] = rho - fuel
    return init


def inputs(case):
    nx, ny, sd, riemann, limiter, extra, _ = case
    d = {"mesh.nx": nx, "mesh.ny": ny, "compressible.limiter": limiter, "compressible.riemann": riemann,
         "compressible.cvisc": 0.1, "driver.cfl": 0.8, "driver.tmax": 1.e3, "driver.max_steps": 1000000,
         "driver.verbose": 0, "vis.dovis": 0, "io.do_io": 0}
    d.update(sd)
    d.update(extra)
    return d


def make(case, seed, extra, fuel_scale=1.0, problem=None, problem_params=None, inputs_dict=None):
    ifc.states = PATCHED_STATES if extra else ORIGINAL_STATES
    p = Pyro("compressible")
    p.solver = types.SimpleNamespace(Simulation=scalar_sim(extra))
    p.add_problem("rough", problem or rough(seed, case[6], fuel_scale), problem_params=problem_params or {})
    p.initialize_problem("rough", inputs_dict=inputs_dict or inputs(case))
    return p


def data(sim):
    return np.array(sim.cc_data.data)


def run(p):
    dts = []
    for _ in range(NSTEPS):
        p.single_step()
        dts.append(p.sim.dt)
    return np.array(dts), data(p.sim)


def comp_meta(sim):
    rp, g = sim.rp, sim.cc_data.grid
    return np.array([g.nx, g.ny, g.ng, g.dx, g.dy, rp.get_param("eos.gamma"),
                     rp.get_param("compressible.limiter"), rp.get_param("compressible.use_flattening"),
                     rp.get_param("compressible.z0"), rp.get_param("compressible.z1"),
                     rp.get_param("compressible.delta"), rp.get_param("compressible.cvisc"),
                     rp.get_param("compressible.grav"), rp.get_param("driver.cfl")])


def react_ic(name, nx, ny, params, over):
    mod = importlib.import_module(f"pyro.compressible_react.problems.{name}")
    d = {"mesh.nx": nx, "mesh.ny": ny, "driver.verbose": 0, "vis.dovis": 0, "io.do_io": 0}
    d.update(over)
    p = make(None, 0, ("fuel", "ash"), problem=mod.init_data, problem_params=params, inputs_dict=d)
    assert p.sim.cc_data.names == ["density", "energy", "x-momentum", "y-momentum", "fuel", "ash"]
    return data(p.sim)


def main():
    out = {"ncases": np.array(len(CASES))}
    for k, case in enumerate(CASES):
        seed = 900 + k
        pre = f"c{k}_"
        p4 = make(case, seed, ())
        dts4, final4 = run(p4)
        p = make(case, seed, ("fuel", "ash"))
        sim, rp = p.sim, p.sim.rp
        ng = sim.cc_data.grid.ng
        assert sim.cc_data.names == ["density", "energy", "x-momentum", "y-momentum", "fuel", "ash"]
        out[pre + "ic"] = data(sim)
        out[pre + "dts"], out[pre + "final"] = run(p)
        I = (slice(ng, -ng), slice(ng, -ng))
        assert np.all(np.isfinite(out[pre + "final"][I]))
        out[pre + "meta"] = comp_meta(sim)
        out[pre + "bc"] = np.array([rp.get_param(s) for s in SIDES])
        out[pre + "riemann"] = np.array(rp.get_param("compressible.riemann"))
        out[pre + "drv"] = np.array([rp.get_param("driver.init_tstep_factor"),
                                     rp.get_param("driver.max_dt_change")])
        scalar_runs = [(out[pre + "dts"], out[pre + "final"])]
        if k in PROPERTY_CASES:
            dts1, f1 = run(make(case, seed, ("fuel",)))
            dtsh, fh = run(make(case, seed, ("fuel", "ash"), fuel_scale=0.5))
            scalar_runs += [(dts1, f1), (dtsh, fh)]
            out[pre + "f1_final"], out[pre + "h_final"] = f1, fh
            # (b), (c): on the whole array -- the ghost cells are images of interior cells
            assert np.array_equal(fh[..., 4], 0.5 * out[pre + "final"][..., 4]), (k, "halving")
            assert np.array_equal(f1[..., 4], out[pre + "final"][..., 4]), (k, "fuel alone")
            assert np.abs(out[pre + "final"][I][..., 4]).max() > 0.1
        for dts, fin in scalar_runs:    # (a)
            assert np.array_equal(dts, dts4), (k, dts, dts4)
            assert np.array_equal(fin[..., :4], final4), (k, "hydro planes")
        moved = np.abs(out[pre + "final"][I] - out[pre + "ic"][I]).max(axis=(0, 1))
        print(pre, case[0], case[1], case[3], "limiter", case[4], "dts", out[pre + "dts"], "moved", moved)
    out["react_flame_ic"] = react_ic("flame", 32, 32, {}, {})
    out["react_rt_ic"] = react_ic("rt", 16, 48, {"rt.dens1": 1.0, "rt.dens2": 2.0, "rt.amp": 1.0,
                                                "rt.sigma": 0.1, "rt.p0": 10.0},
                                  {"compressible.grav": -1.0, "mesh.xmax": 1.0, "mesh.ymax": 3.0, "rt.amp": 0.25})
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "comp_scalars.npz")
    extra = os.environ.get("COMP_SCALARS_EXTRA")    # arrays recorded elsewhere (sedov64_* of the 4-variable run)
    if extra:
        out.update(dict(np.load(extra)))
    elif os.path.exists(path):
        old = np.load(path)
        out.update({n: old[n] for n in old.files if n.startswith("sedov64_")})
    tmp = os.path.join(tempfile.mkdtemp(), "comp_scalars.npz")
    np.savez_compressed(tmp, **out)
    assert os.path.getsize(tmp) < 1000 * 1000, os.path.getsize(tmp)     # (d)
    shutil.move(tmp, path)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
