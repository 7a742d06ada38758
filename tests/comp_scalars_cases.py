"""Shared pieces of tests/test_comp_scalars.py: the recorded reference runs of
tests/golden/comp_scalars.npz (tools/gen_comp_scalars_golden.py), rough states at the sizes the
property tests add, and the drivers that step a state with passive scalars through the C ABI."""
import numpy as np

from helpers import DtPolicy
from oracle import orc
from pyro2_amd import device

NAMES = ["density", "energy", "x-momentum", "y-momentum", "fuel", "ash"]
NCASES = 5
PROPERTY_CASES = (0, 1, 2)       # the cases whose one-scalar and halved runs are recorded
NSTEPS = 3
# the project's compressible tolerance of the contracted build, element-wise (tests/conftest.py
# elementwise_err with the per-variable floors of comp_floors)
TOL_FAST = 1e-10


def var_bcs(bcs, nvar):
    """boundary codes per variable: the four hydro ones, then the scalars with the density's
    (compressible/simulation.py:223-231: registered with `bc`, even at reflecting sides)"""
    vb = [list(r) for r in orc.comp_var_bcs(bcs)]
    return vb + [list(vb[0]) for _ in range(nvar - 4)]


def state(dev, nx, ny, bcs, nvar, ng=4):
    return device.DeviceState(dev, nx, ny, ng, var_bcs(bcs, nvar))


def params(meta, bcs, riemann="HLLC", **kw):
    nx, ny, ng, dx, dy, gamma, lim, flat, z0, z1, delta, cvisc, grav, cfl = meta
    solid = [int(b in ("reflect", "reflect-even", "reflect-odd", "dirichlet")) for b in bcs]
    kw.setdefault("kernel_set", 1)
    return device.make_comp_params(dx, dy, gamma=gamma, limiter=int(lim), use_flattening=int(flat),
                                   z0=z0, z1=z1, delta=delta, cvisc=cvisc, grav=grav, riemann=riemann,
                                   solid_xl=solid[0], solid_yl=solid[2], **kw), float(cfl)


def run(dev, ic, meta, bcs, riemann="HLLC", nsteps=NSTEPS, drv=(0.01, 2.0), fuse_fill=False, **kw):
    """nsteps of the driver's loop (fill, dt policy, step) on a state of ic.shape[2] planes;
    fuse_fill: the fill is left to the step kernel from the second step on (the first dt
    needs filled ghost cells)"""
    nx, ny, ng = int(meta[0]), int(meta[1]), int(meta[2])
    P, cfl = params(meta, bcs, riemann, **kw)
    s = state(dev, nx, ny, bcs, ic.shape[2], ng)
    s.upload(np.ascontiguousarray(ic))
    pol, dts = DtPolicy(1.e30, drv[0], drv[1]), []
    for n in range(nsteps):
        P.fuse_fill = int(fuse_fill and n > 0)
        if not P.fuse_fill:
            s.fill_bc()
        dt = pol(s.comp_dt(P, cfl))
        s.comp_step(P, dt)
        pol.advance(dt)
        dts.append(dt)
    return s.download(), dts


def golden_case(g, k):
    pre = f"c{k}_"
    return dict(ic=g[pre + "ic"], meta=g[pre + "meta"], bcs=[str(b) for b in g[pre + "bc"]],
                riemann=str(g[pre + "riemann"]), drv=tuple(g[pre + "drv"]), dts=g[pre + "dts"],
                final=g[pre + "final"])


def rough_state(nx, ny, seed, jump=None, ng=4):
    """the goldens' kind of state at any size: rho, E = 1 + U(-0.3, 0.3) (E + 2), momenta
    U(-0.3, 0.3), an energy jump of 10^3 from cell `jump` on; fuel = rho U(0, 1), ash = rho - fuel"""
    rng = np.random.default_rng(seed)
    r = rng.random((5, nx + 2 * ng, ny + 2 * ng))
    U = np.empty((nx + 2 * ng, ny + 2 * ng, 6))
    U[..., 0] = 1.0 + 0.3 * (2.0 * r[0] - 1.0)
    U[..., 1] = 3.0 + 0.3 * (2.0 * r[1] - 1.0)
    if jump is not None:
        U[ng + jump[0]:, ng + jump[1]:, 1] *= 1.e3
    U[..., 2] = 0.3 * (2.0 * r[2] - 1.0)
    U[..., 3] = 0.3 * (2.0 * r[3] - 1.0)
    U[..., 4] = U[..., 0] * r[4]
    U[..., 5] = U[..., 0] - U[..., 4]
    meta = np.array([nx, ny, ng, 1.0 / nx, 1.0 / ny, 1.4, 2, 1, 0.75, 0.85, 0.33, 0.1, 0.0, 0.8])
    return U, meta


# (label, golden case or None, (nx, ny, sides, solver, limiter, flattening, grav, jump), GPU only)
_X = ["outflow"] * 4
PROPERTY_SHAPES = [
    ("c0", 0, None, False), ("c1", 1, None, False), ("c2", 2, None, False), ("c3", 3, None, False),
    ("c4", 4, None, False),
    # 8 x 8 tiles: the XCD renumbering of the tile walk is active; 90 ragged tiles: identity walk
    ("112x240", None, (112, 240, _X, "HLLC", 2, 1, 0.0, (56, 120)), True),
    ("127x250", None, (127, 250, ["reflect", "reflect", "periodic", "periodic"], "HLLC_lm", 1, 1, -1.0,
                 (70, 150)), True),
]


def property_case(g, label):
    """ic (6 planes), meta, sides, solver, drv of a property shape"""
    _, k, spec, _ = next(c for c in PROPERTY_SHAPES if c[0] == label)
    if k is not None:
        c = golden_case(g, k)
        return c["ic"], c["meta"], c["bcs"], c["riemann"], c["drv"]
    nx, ny, bcs, riemann, lim, flat, grav, jump = spec
    U, meta = rough_state(nx, ny, 7000 + nx, jump)
    meta[6], meta[7], meta[12] = lim, flat, grav
    return U, meta, bcs, riemann, (0.01, 2.0)
