"""The case table of the invalid-state contract (tests/test_invalid_state.py,
oracle/gen_invalid_golden.py): base states and one-cell perturbations of them.

The reference refuses to step a compressible state whose interior has
min(rho) <= 0 or min(e) <= 0 (compressible/simulation.py:68-71, numpy minima:
a NaN fails too).  A case puts one value into one interior cell of a smooth,
moving state; the generator asks the reference for its verdict and stores it
beside the case descriptor in tests/golden/comp_invalid_cases.npz -- the table
here and the fixture are compared row by row before any verdict is used.

State layout: (qx, qy, 4) = density, energy, x-momentum, y-momentum; i (first
axis) is the row the row-marching kernels march along, j the contiguous one.
"""
import numpy as np

NG = 4
GAMMA = 1.4
SEED = 20261

# The Cartesian grid: 47 rows x 130 columns.  Column strips of the row-marching kernels are 56
# wide (comp_wave.hip WOUT): 56 + 56 + 18.  Row strips: 8 rows by the library's choice (5 x 8 + 7),
# 11 rows under march_rows = 11 (11 + 11 + 11 + 14: a last strip shorter than the ghost width joins
# its predecessor, wave_geometry).  The 2-d tile kernel updates 14 x 30 cells per tile
# (comp_fused.hip FTI x FTJ): 14 + 14 + 14 + 5 rows, 30 + 30 + 30 + 30 + 10 columns.
NX, NY = 47, 130
COL_STRIP = 56
ROW_STRIPS = (8, 11)
TILE = (14, 30)

SMALL_DENS = (-1.e200, 1.e-4)

KINDS = ("rho_neg", "rho_pzero", "rho_nzero", "e_neg", "e_zero", "nan_dens", "nan_ener",
         "nan_xmom", "nan_ymom", "nan_dens_rest", "rho_pinf", "ener_ninf", "ok_small_e", "ok_small_rho")
SWEPT_KINDS = ("nan_ener", "rho_neg")        # these two visit every position


def positions(nx=NX, ny=NY):
    """interior (i, j), 0-based, of the cells a bad value is put into: the first one is the
    mid-grid cell every kind visits"""
    im, jm = nx // 2, ny // 2
    pos = [(im, jm)]
    pos += [(0, 0), (0, ny - 1), (nx - 1, 0), (nx - 1, ny - 1)]
    pos += [(0, jm), (nx - 1, jm), (im, 0), (im, ny - 1)]
    seams_j = set(range(COL_STRIP, ny, COL_STRIP)) | set(range(TILE[1], ny, TILE[1]))
    seams_i = set(range(TILE[0], nx, TILE[0]))
    for L in ROW_STRIPS:
        n = (nx + L - 1) // L
        if n > 1 and nx - (n - 1) * L < NG:
            n -= 1
        seams_i |= {k * L for k in range(1, n)}
    for j in sorted(seams_j):
        pos += [(im, j - 1), (im, j)]
    for i in sorted(seams_i):
        pos += [(i - 1, jm), (i, jm)]
    out = []
    for p in pos:
        if p not in out:
            out.append(p)
    return out


def sph_positions(nx, ny):
    """the same idea on the small SphericalPolar grids of the golden file (one column strip, the
    tile seams at 14 and 30, the 8- and 11-row strips)"""
    im, jm = nx // 2, ny // 2
    pos = [(im, jm), (0, 0), (nx - 1, ny - 1), (0, jm), (im, ny - 1)]
    for i in (8, 11, 14):
        if i < nx:
            pos += [(i - 1, jm), (i, jm)]
    return pos


def base_state(nx=NX, ny=NY, seed=SEED):
    """a smooth state that moves everywhere: rho in [0.8, 1.2], u around 0.5, v around 0.25,
    p in [0.9, 1.1]; ghost cells hold the same functions (any boundary rule may overwrite them)"""
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0.0, 2.0 * np.pi, 4)
    x = (np.arange(nx + 2 * NG) + 0.5 - NG) / nx
    y = (np.arange(ny + 2 * NG) + 0.5 - NG) / ny
    X, Y = np.meshgrid(x, y, indexing="ij")
    rho = 1.0 + 0.2 * np.sin(2 * np.pi * (X + 2 * Y) + ph[0])
    u = 0.5 + 0.1 * np.cos(2 * np.pi * (2 * X - Y) + ph[1])
    v = 0.25 + 0.1 * np.sin(2 * np.pi * (X + Y) + ph[2])
    p = 1.0 + 0.1 * np.cos(2 * np.pi * (X - 3 * Y) + ph[3])
    U = np.empty(X.shape + (4,))
    U[..., 0] = rho
    U[..., 1] = p / (GAMMA - 1.0) + 0.5 * rho * (u * u + v * v)
    U[..., 2] = rho * u
    U[..., 3] = rho * v
    return U


def apply_case(U, kind, i, j, ng=NG):
    """put the case's value into interior cell (i, j) of a copy of U"""
    U = U.copy()
    c = U[ng + i, ng + j]            # a view: density, energy, x-momentum, y-momentum
    rho, E, mx, my = (float(a) for a in c)
    ke = 0.5 * (mx * mx + my * my) / rho
    if kind == "rho_neg":
        c[0] = -rho
    elif kind == "rho_pzero":
        c[0] = 0.0
    elif kind == "rho_nzero":
        c[0] = -0.0
    elif kind == "e_neg":
        c[1] = 0.5 * ke
    elif kind == "e_zero":
        # rho = 2, u = 1/2, v = 1/4: E = rho (u^2 + v^2) / 2 = 5/16 and e = 0.0, all of it exact
        c[:] = (2.0, 0.3125, 1.0, 0.5)
    elif kind == "nan_dens_rest":
        # a NaN density in a cell at rest: a floor that absorbed the NaN would leave a VALID cell
        # (in a moving cell the floored density makes e negative, and the case is caught by accident)
        c[:] = (np.nan, E - ke, 0.0, 0.0)
    elif kind.startswith("nan_"):
        c[("dens", "ener", "xmom", "ymom").index(kind[4:])] = np.nan
    elif kind == "rho_pinf":
        c[0] = np.inf
    elif kind == "ener_ninf":
        c[1] = -np.inf
    elif kind == "ok_small_e":
        # valid, just: e = 1e-6 of the specific kinetic energy
        c[1] = ke * (1.0 + 1.e-6)
    elif kind == "ok_small_rho":
        # valid, just: rho = 1e-12 with the cell's velocity and specific energy
        c[:] = np.array([rho, E, mx, my]) * (1.e-12 / rho)
    else:
        raise ValueError(kind)
    return U


def case_table(npos=None):
    """[(kind, i, j)]: every kind at the mid-grid cell, the two swept kinds at every position"""
    pos = positions() if npos is None else npos
    cases = [(k, *pos[0]) for k in KINDS]
    for k in SWEPT_KINDS:
        cases += [(k, i, j) for (i, j) in pos[1:]]
    return cases


def numpy_verdict(U, small_dens, ng=NG):
    """the reference's verdict restated (clean_state, simulation.py:452-456, and the head of
    cons_to_prim, :49-71): 1 = the assert fires"""
    U = U.copy()
    I = (slice(ng, -ng), slice(ng, -ng))
    U[I + (0,)] = np.maximum(U[I + (0,)], small_dens)
    rho = U[..., 0]
    nz = rho != 0.0
    with np.errstate(all="ignore"):
        u = np.divide(U[..., 2], rho, out=np.zeros_like(rho), where=nz)
        v = np.divide(U[..., 3], rho, out=np.zeros_like(rho), where=nz)
        e = np.divide(U[..., 1] - 0.5 * rho * (u ** 2 + v ** 2), rho, out=np.zeros_like(rho), where=nz)
        return int(not (e[I].min() > 0.0 and rho[I].min() > 0.0))


# ---------------------------------------------------------------------------
# a run that the scheme itself makes invalid: colliding supersonic streams
# ---------------------------------------------------------------------------
COLLIDE_MACH = (10.0, 100.0)
COLLIDE_BCS = ("outflow",) * 4
COLLIDE_DRV = (0.01, 2.0)        # init_tstep_factor, max_dt_change
COLLIDE_CFL = 0.8


def collide_state(mach, nx=NX, ny=NY):
    """rho = 1 + 0.2 sin(7x + 3y), u = M c tanh((x - 0.37) / 0.02), v = M c tanh((y - 0.61) / 0.03),
    p = p0 = 1e-2, c = sqrt(gamma p0), on the unit square"""
    p0 = 1.e-2
    c = np.sqrt(GAMMA * p0)
    x = (np.arange(nx + 2 * NG) + 0.5 - NG) / nx
    y = (np.arange(ny + 2 * NG) + 0.5 - NG) / ny
    X, Y = np.meshgrid(x, y, indexing="ij")
    rho = 1.0 + 0.2 * np.sin(7.0 * X + 3.0 * Y)
    u = mach * c * np.tanh((X - 0.37) / 0.02)
    v = mach * c * np.tanh((Y - 0.61) / 0.03)
    U = np.empty(X.shape + (4,))
    U[..., 0] = rho
    U[..., 1] = p0 / (GAMMA - 1.0) + 0.5 * rho * (u * u + v * v)
    U[..., 2] = rho * u
    U[..., 3] = rho * v
    return U


def collide_meta(nx=NX, ny=NY):
    """the meta row of helpers.meta_to_params: limiter 2, flattening on, no gravity"""
    return np.array([nx, ny, NG, 1.0 / nx, 1.0 / ny, GAMMA, 2, 1, 0.75, 0.85, 0.33, 0.1, 0.0,
                     COLLIDE_CFL])


def margin(U, ng=NG):
    """min(e) / max(E / rho) over the interior: how far the state is from the assert"""
    I = U[ng:-ng, ng:-ng]
    rho, E, mx, my = (I[..., n] for n in range(4))
    e = (E - 0.5 * (mx * mx + my * my) / rho) / rho
    return float(e.min() / (E / rho).max())
