"""Generate tests/golden/comp_floor_grav.npz: one step of THE REFERENCE (pyro2) from a state with
interior densities below compressible.small_dens, under gravity, beside a periodic side -- the case
in which the gravity source of a ghost cell that is the image of a floored cell decides the result
(tests/test_ctu_oracle.py, DESIGN.md 3: finding A).

TEST INFRASTRUCTURE ONLY.  Run where the reference is importable, as oracle/gen_golden.py (same
shim, same interpreter):

    MPLBACKEND=Agg PYTHONPATH=oracle/shim:<reference> python oracle/gen_ctu_floor_golden.py

The reference (compressible/simulation.py:296, 452-456) floors the interior in place and leaves the
ghost cells as the fill left them; apply_source_terms (unsplit_fluxes.py:295-306) evaluates the
source over the whole array and then fills the source's ghost cells from its interior by the
boundary rules -- so the source of a ghost cell is that of the FLOORED interior cell it mirrors.

Stored: the grid and the parameters, the filled input, dt, the reference's state after evolve().
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
os.chdir(tempfile.mkdtemp())  # Pyro writes inputs.auto into cwd

try:        # the reference imports h5py at import time (util/io_pyro.py); no file is read or written here
    import h5py  # noqa: F401
except ImportError:
    import types
    sys.modules["h5py"] = types.ModuleType("h5py")

import pyro                                           # noqa: E402
from pyro.pyro_sim import Pyro                         # noqa: E402

assert not os.path.abspath(pyro.__file__).startswith(ROOT + os.sep), "this is not the reference"
sys.path += [ROOT, os.path.join(ROOT, "tests")]

import sph_cases as sc                                 # noqa: E402
from oracle import orc                                 # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "comp_floor_grav.npz")
NX, NY, NG = 8, 57, 4
XMAX, YMAX = 1.0, 1.5
BCS = ("reflect", "outflow", "periodic", "periodic")
LIMITER, FLATTEN, GRAV, SMALL_DENS, CFL = 2, 1, -0.3, 0.05, 0.8
ROWS, COLS = [4], [30]


def put(sim, U):
    iv = sim.ivars
    d = sim.cc_data.data
    for n, m in enumerate((iv.idens, iv.iener, iv.ixmom, iv.iymom)):
        d[:, :, m] = U[:, :, n]


def get(sim):
    iv = sim.ivars
    d = sim.cc_data.data
    return np.stack([np.array(d[:, :, m]) for m in (iv.idens, iv.iener, iv.ixmom, iv.iymom)], axis=-1)


def main():
    p = Pyro("compressible")
    p.initialize_problem("sedov", inputs_dict={
        "mesh.nx": NX, "mesh.ny": NY, "mesh.xmax": XMAX, "mesh.ymax": YMAX, "eos.gamma": sc.GAMMA,
        "driver.cfl": CFL, "compressible.small_dens": SMALL_DENS, "compressible.grav": GRAV,
        "compressible.limiter": LIMITER, "compressible.use_flattening": FLATTEN,
        "compressible.riemann": "HLLC",
        "mesh.xlboundary": BCS[0], "mesh.xrboundary": BCS[1],
        "mesh.ylboundary": BCS[2], "mesh.yrboundary": BCS[3]})
    sim = p.sim
    g = sim.cc_data.grid
    assert (g.nx, g.ny, g.ng) == (NX, NY, NG) and g.dx == XMAX / NX and g.dy == YMAX / NY
    U0 = sc.make_state("floor", NX, NY, ROWS, COLS)
    put(sim, U0)
    sim.cc_data.fill_BC_all()
    U0 = get(sim)
    I = (slice(NG, -NG), slice(NG, -NG))
    floored = np.argwhere(U0[I][..., 0] < SMALL_DENS)
    assert [1, 0] in floored.tolist() and [NX - 2, NY - 1] in floored.tolist(), floored
    sim.method_compute_timestep()       # (compute_timestep would apply the first step's init_tstep_factor)
    dt = float(sim.dt)
    assert dt == orc.comp_dt(U0, NX, NY, NG, g.dx, g.dy, sc.GAMMA, CFL)
    sim.evolve()
    U1 = get(sim)
    assert np.isfinite(U1).all()
    # the ghost cells are as the fill left them: not floored
    assert np.array_equal(U1[:, :NG], U0[:, :NG]) and U0[NG + 1, NG + NY, 0] < SMALL_DENS
    np.savez_compressed(OUT, grid=np.array([NX, NY, NG]), dxdy=np.array([g.dx, g.dy]), bc=np.array(BCS),
                        params=np.array([sc.GAMMA, LIMITER, FLATTEN, GRAV, SMALL_DENS, CFL]),
                        seams=np.array([ROWS[0], COLS[0]]), U0=U0, dt=np.array(dt), U1=U1)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
