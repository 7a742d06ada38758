"""Generate tests/golden/comp_invalid_cases.npz by asking THE REFERENCE (pyro2)
for its verdict on every case of tests/invalid_cases.py.

TEST INFRASTRUCTURE ONLY.  Run where the reference is importable, as
oracle/gen_golden.py (same shim, same interpreter):

    MPLBACKEND=Agg PYTHONPATH=oracle/shim:<reference> python oracle/gen_invalid_golden.py

A case is put into the reference Simulation's cc_data; the verdict is what the
reference's own clean_state + cons_to_prim (the first thing evolve() does,
compressible/simulation.py:296 and unsplit_fluxes.py:160) say under
try / except AssertionError: 1 = the assert fired.  A case the reference
accepts is then stepped with the reference's evolve(), and one whose step
leaves non-finite values is NOT recorded (it has no defined outcome to hold a
kernel to: E = +inf is such a case, accepted by the assert, NaN one step on --
it is not in the table for that reason).

Nothing but case descriptors, verdicts and a few scalars is stored: no states.
The colliding-streams runs are recorded from the C oracle (step index, dt
sequence, margins) and, where the reference gets that far in reasonable time,
checked against the reference's own run.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
os.chdir(tempfile.mkdtemp())  # Pyro writes inputs.auto into cwd

import pyro.compressible as comp                       # noqa: E402
import pyro                                           # noqa: E402
from pyro.pyro_sim import Pyro                         # noqa: E402

# (behind the reference on the path: this repository has a package called pyro of its own)
assert not os.path.abspath(pyro.__file__).startswith(ROOT + os.sep), "this is not the reference"
sys.path += [ROOT, os.path.join(ROOT, "tests")]

import invalid_cases as ic                             # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "comp_invalid_cases.npz")


def put(sim, U):
    iv = sim.ivars
    d = sim.cc_data.data
    for n, m in enumerate((iv.idens, iv.iener, iv.ixmom, iv.iymom)):
        d[:, :, m] = U[:, :, n]


def get(sim):
    iv = sim.ivars
    d = sim.cc_data.data
    return np.stack([np.array(d[:, :, m]) for m in (iv.idens, iv.iener, iv.ixmom, iv.iymom)], axis=-1)


def verdict(sim, U, step):
    """(1 = the reference's assert fires, finite after a step of the reference?)"""
    put(sim, U)
    gamma = sim.rp.get_param("eos.gamma")
    with np.errstate(all="ignore"):
        try:
            sim.clean_state(sim.cc_data.data)
            comp.cons_to_prim(sim.cc_data.data, gamma, sim.ivars, sim.cc_data.grid)
        except AssertionError:
            return 1, True
        if not step:
            return 0, True
        put(sim, U)
        sim.cc_data.fill_BC_all()
        sim.compute_timestep()
        sim.dt *= 0.5
        try:
            sim.evolve()
        except AssertionError:
            raise SystemExit("the reference's evolve() disagrees with its clean_state + cons_to_prim")
        return 0, bool(np.isfinite(get(sim)[ic.NG:-ic.NG, ic.NG:-ic.NG]).all())


def cartesian(small_dens):
    p = Pyro("compressible")
    p.initialize_problem("sedov", inputs_dict={
        "mesh.nx": ic.NX, "mesh.ny": ic.NY, "eos.gamma": ic.GAMMA,
        "compressible.small_dens": small_dens,
        "mesh.xlboundary": "outflow", "mesh.xrboundary": "outflow",
        "mesh.ylboundary": "outflow", "mesh.yrboundary": "outflow"})
    return p.sim


def spherical(small_dens, nx, ny):
    p = Pyro("compressible")
    p.initialize_problem("sedov", inputs_file="inputs.sedov.spherical", inputs_dict={
        "mesh.nx": nx, "mesh.ny": ny, "compressible.small_dens": small_dens})
    assert type(p.sim.cc_data.grid).__name__ == "SphericalPolar"
    return p.sim


def main():
    out = {"seed": np.array(ic.SEED), "grid": np.array([ic.NX, ic.NY, ic.NG]),
           "small_dens": np.array(ic.SMALL_DENS), "kinds": np.array(ic.KINDS)}
    base = ic.base_state()
    cases = ic.case_table()
    rows, verd = [], []
    dropped = []
    for kind, i, j in cases:
        U = ic.apply_case(base, kind, i, j)
        vs = []
        for sd in ic.SMALL_DENS:
            # (stepping the reference costs seconds: the accepted cases are few)
            v, fin = verdict(cartesian(sd), U, step=True)
            assert ic.numpy_verdict(U, sd) == v, (kind, i, j, sd)
            if not fin:
                dropped.append((kind, i, j, sd))
            vs.append(v)
        rows.append((ic.KINDS.index(kind), i, j))
        verd.append(vs)
        print(kind, i, j, vs, flush=True)
    assert not dropped, dropped      # the table holds no case without a defined outcome
    out["cases"] = np.array(rows, dtype=np.int32)
    out["verdict"] = np.array(verd, dtype=np.int8)          # [case, small_dens]

    # SphericalPolar: the reference's sedov set-up of the golden file comp_spherical (case 0),
    # every kind at the first position, the swept kinds at the others
    snx, sny = 48, 24
    sim = spherical(ic.SMALL_DENS[0], snx, sny)
    sbase = get(sim)
    spos = ic.sph_positions(snx, sny)
    srows, sverd = [], []
    for kind, i, j in ic.case_table(spos):
        U = ic.apply_case(sbase, kind, i, j)
        vs = []
        for sd in ic.SMALL_DENS:
            v, fin = verdict(spherical(sd, snx, sny), U, step=False)
            vs.append(v)
        srows.append((ic.KINDS.index(kind), i, j))
        sverd.append(vs)
    out["sph_grid"] = np.array([snx, sny])
    out["sph_cases"] = np.array(srows, dtype=np.int32)
    out["sph_verdict"] = np.array(sverd, dtype=np.int8)

    # the colliding streams: step index, dts and margins from the C oracle ...
    from helpers import DtPolicy, meta_to_params
    from oracle import orc
    meta = ic.collide_meta()
    for m, mach in enumerate(ic.COLLIDE_MACH):
        P, cfl = meta_to_params(meta, ic.COLLIDE_BCS)
        U = ic.collide_state(mach)
        pol = DtPolicy(1.e30, *ic.COLLIDE_DRV)
        dts, margins = [], []
        while True:
            orc.comp_fill_bc(U, P.nx, P.ny, P.ng, ic.COLLIDE_BCS, P.gamma, P.grav, P.dy)
            dt = pol(orc.comp_dt(U, P.nx, P.ny, P.ng, P.dx, P.dy, P.gamma, cfl))
            margins.append(ic.margin(U))
            V = U.copy()
            rc, _ = orc.comp_step(V, P, dt)
            if rc:
                break
            U = V
            pol.advance(dt)
            dts.append(dt)
            assert pol.n < 40
        k = pol.n
        out[f"collide{m}_mach"] = np.array(mach)
        out[f"collide{m}_k"] = np.array(k)
        out[f"collide{m}_dts"] = np.array(dts)
        out[f"collide{m}_margins"] = np.array(margins[-2:])    # last accepted input, rejected state
        print("colliding streams M", mach, "good steps", k, "margins", margins[-2:], flush=True)
        # ... and the reference's own run: the assert fires entering the same step, after the same dts
        p = Pyro("compressible")
        p.initialize_problem("sedov", inputs_dict={
            "mesh.nx": ic.NX, "mesh.ny": ic.NY, "eos.gamma": ic.GAMMA, "driver.cfl": ic.COLLIDE_CFL,
            "driver.init_tstep_factor": ic.COLLIDE_DRV[0], "driver.max_dt_change": ic.COLLIDE_DRV[1],
            "driver.tmax": 1.e30, "driver.max_steps": 1000,
            "compressible.limiter": 2, "compressible.use_flattening": 1, "compressible.grav": 0.0,
            "mesh.xlboundary": "outflow", "mesh.xrboundary": "outflow",
            "mesh.ylboundary": "outflow", "mesh.yrboundary": "outflow"})
        put(p.sim, ic.collide_state(mach))
        rdts = []
        with np.errstate(all="ignore"):
            try:
                for _ in range(k + 1):
                    p.single_step()
                    rdts.append(p.sim.dt)
                raise SystemExit("the reference took the step the oracle rejects")
            except AssertionError:
                pass
        assert p.sim.n == k and len(rdts) == k, (p.sim.n, k)
        assert np.abs(np.array(rdts) / np.array(dts) - 1).max() < 1e-12
        out[f"collide{m}_ref_k"] = np.array(p.sim.n)
        print("   the reference: assert entering step", p.sim.n + 1, flush=True)

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
