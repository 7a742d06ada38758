"""Shapes, states and parameters for the SphericalPolar step kernels against the C oracle
(tests/test_sph_oracle.py).

Shapes: one for every path of k_sph_wave's unit decoding (csrc/comp_sph_wave.hip: sphw_geometry,
csrc/wave_march.h), for 4 compute units (the emulated device) and 256 (the MI355X) -- PATHS names
them and test_sph_oracle.py::test_wave_geometry_reaches_every_path holds the list to the library's
own geometry call -- with the column counts around 1, 2 and 3 times the 56 updated columns of a
wavefront and the row counts around the 32 rows from which the library cuts row strips.

States (qx, qy, 4) = (density, energy, r momentum, theta momentum) over the WHOLE array; the test
then fills the ghost frame with the oracle's fill for the case's boundary types.  All seeded."""
import numpy as np

NG = 4
SWOUT = 56            # columns a wavefront of k_sph_wave updates
GAMMA = 1.4
CFL = 0.8
DOMAIN = (1.0, 1.9, 0.785, 2.355)       # xmin (xmin - ng dx >= 0 down to nx = 4), xmax, ymin, ymax
SMALL_DENS = 0.05                       # of the `floor` state's cases
GRAV = -0.3                             # of the cases with radial gravity

# (nx, ny, march_rows)
SHAPES = [(4, 4, 0), (31, 55, 0), (32, 64, 0), (8, 169, 0),
          (35, 112, 0), (33, 56, 5), (35, 60, 11),
          (70, 57, 11),
          (5, 57, 1), (12, 113, 3), (66, 4, 11),
          (36, 57, 0), (40, 113, 0), (70, 120, 0),
          (70, 58, 1)]
MIXED_NX = 36         # rows of the grids with cut and regular column strips in one launch (two row strips)
NOPRIO_NX = 70        # rows of the grid of 1-row strips with more wavefronts than two rounds of slots


def pick_mixed(geometry, cus):
    """the smallest MIXED_NX x ny grid (ny = 56 ncb - 3: a ragged last column strip) that has, on
    `cus` compute units, at least two cut and at least two regular column strips in one launch;
    geometry(nx, ny, cus, march_rows) -> dict of device.sph_wave_geometry"""
    for ncb in range(2, 8 * cus):
        ny = SWOUT * ncb - 3
        g = geometry(MIXED_NX, ny, cus, 0)
        if 2 <= g["n_extra"] <= g["col_strips"] - 2:
            return (MIXED_NX, ny, 0)
    raise AssertionError("no grid with cut and regular column strips")


def pick_noprio(geometry, cus):
    """the smallest NOPRIO_NX x ny grid (ny = 56 ncb + 2) of 1-row strips with more wavefronts than
    two rounds of resident ones on `cus` compute units (prio_duty == 0)"""
    for ncb in range(1, 8 * cus):
        ny = SWOUT * (ncb - 1) + 2
        g = geometry(NOPRIO_NX, ny, cus, 1)
        if g["prio_duty"] == 0:
            return (NOPRIO_NX, ny, 1)
    raise AssertionError("no grid without priority turns")


# path of the unit decoding -> {compute units: shapes that must take it}; "mixed" and "noprio" stand
# for pick_mixed / pick_noprio of that device (on 256 compute units they are large: GPU only)
PATHS = {
    "one_strip": {cus: [(4, 4, 0), (31, 55, 0), (32, 64, 0), (8, 169, 0)] for cus in (4, 256)},
    "joined_last": {cus: [(35, 112, 0), (33, 56, 5), (35, 60, 11)] for cus in (4, 256)},
    "last_ng": {cus: [(70, 57, 11)] for cus in (4, 256)},
    "march_rows": {cus: [(33, 56, 5), (35, 60, 11), (70, 57, 11), (5, 57, 1), (12, 113, 3), (66, 4, 11), (70, 58, 1)]
                   for cus in (4, 256)},
    "one_row_strips": {cus: [(5, 57, 1), (70, 58, 1)] for cus in (4, 256)},
    "all_cut": {cus: [(36, 57, 0), (40, 113, 0), (70, 120, 0)] for cus in (4, 256)},
    "cut_and_regular": {4: ["mixed"], 256: ["mixed"]},
    "no_priority": {4: [(70, 58, 1)], 256: ["noprio"]},
}


def strips_of(geo, nx):
    """rows [i0, i1) (offsets from ilo) of the row strips of a geometry (device.sph_wave_geometry):
    (regular, cut) -- regular: L rows each, the last one to the end (it holds a joined short tail);
    cut: the row_strips + 1 equal parts of the column strips [0, n_extra)"""
    L, nsb, ne = geo["rows_per_strip"], geo["row_strips"], geo["n_extra"]
    regular = [(sb * L, nx if sb == nsb - 1 else sb * L + L) for sb in range(nsb)]
    cut = [(sb * nx // (nsb + 1), (sb + 1) * nx // (nsb + 1)) for sb in range(nsb + 1)] if ne else []
    return regular, cut


def paths_of(geo, nx, march_rows):
    """the names of PATHS a geometry takes"""
    L, nsb, ne, ncb = geo["rows_per_strip"], geo["row_strips"], geo["n_extra"], geo["col_strips"]
    regular, _ = strips_of(geo, nx)
    last = regular[-1][1] - regular[-1][0]
    out = set()
    if ne == 0:
        if nsb == 1 and nx <= 32 and march_rows == 0:
            out.add("one_strip")
        if last > L:
            out.add("joined_last")
        if nsb > 1 and last == NG:
            out.add("last_ng")
        if march_rows > 0 and nsb > 1:
            out.add("march_rows")
            if L == 1:
                out.add("one_row_strips")
    else:
        out.add("all_cut" if ne == ncb else "cut_and_regular")
    if geo["prio_duty"] == 0:
        out.add("no_priority")
    return out


def row_seams(nx, geos):
    """first rows (offsets from ilo) of the row strips of the given geometries"""
    out = set()
    for geo in geos:
        regular, cut = strips_of(geo, nx)
        out |= {a for a, _ in regular + cut if 0 < a < nx}
    return sorted(out)


def col_seams(ny):
    """first columns (offsets from jlo) of the column strips behind the first"""
    return list(range(SWOUT, ny, SWOUT))


# ---------------------------------------------------------------- parameters
BCS = [("reflect-odd", "outflow", "outflow", "outflow"),        # (the Sedov set-up's)
       ("outflow", "reflect", "periodic", "periodic"),
       ("reflect", "reflect", "reflect", "reflect")]
STATES = ("smooth", "super", "zeros", "sedov", "floor")
# (limiter, use_flattening, grav, geometry with the 1-d factors rowf / colf): every value of each,
# both template instances STD (limiter 2 with flattening, or not) and FAC of k_sph_wave, and each
# pair of (STD, FAC)
PARAMS = [(2, 1, 0.0, 1), (2, 1, GRAV, 0), (0, 1, 0.0, 1), (1, 0, GRAV, 1), (2, 0, 0.0, 0), (0, 0, GRAV, 0),
          (1, 1, GRAV, 1)]


def cases_of(shape, n_shape):
    """the cases of a shape: every state, the boundary mixes and the parameter rows taken in turn
    (the offsets move with the shape's place in the list, so that over the list every state meets
    every boundary mix, and every parameter row every kind of shape): (state, bcs, limiter,
    use_flattening, grav, fac, small_dens)"""
    out = []
    for n, kind in enumerate(STATES):
        lim, flat, grav, fac = PARAMS[(n_shape * 3 + n) % len(PARAMS)]
        out.append((kind, BCS[(n_shape + n) % len(BCS)], lim, flat, grav, fac,
                    SMALL_DENS if kind == "floor" else -1.e200))
    return out


def solid(bcs):
    return [int(b in ("reflect", "reflect-even", "reflect-odd", "dirichlet")) for b in bcs]


def grid_of(nx, ny):
    from pyro2_amd.mesh import patch
    return patch.SphericalPolar(nx, ny, ng=NG, xmin=DOMAIN[0], xmax=DOMAIN[1], ymin=DOMAIN[2], ymax=DOMAIN[3])


def state_seed(nx, ny, kind):
    kind = "floor" if kind == "floor_wall" else kind
    return 1000 * (1 + STATES.index(kind)) + 7 * nx + ny


# ---------------------------------------------------------------- states
def cons(rho, u, v, p):
    E = p / (GAMMA - 1.0) + 0.5 * rho * (u * u + v * v)
    return np.ascontiguousarray(np.stack([rho, E, rho * u, rho * v], axis=-1))


def smooth_prims(nx, ny, seed):
    rng = np.random.default_rng(seed)
    qx, qy = nx + 2 * NG, ny + 2 * NG
    x = np.arange(qx)[:, None] / max(nx, 16)
    y = np.arange(qy)[None, :] / max(ny, 16)
    rho = 1.0 + 0.3 * np.sin(6 * x) * np.cos(4 * y) + 0.05 * rng.random((qx, qy))
    u = 0.4 * np.cos(3 * x + y) + 0.0 * rho
    v = -0.5 * np.sin(5 * y - x) + 0.0 * rho
    p = 1.0 + 0.2 * np.cos(5 * x - 2 * y) + 0.02 * rng.random((qx, qy))
    return rho, u, v, p


def make_state(kind, nx, ny, rows=(), cols=()):
    """a state (qx, qy, 4) of the given kind; rows / cols: first rows / columns (offsets from ilo /
    jlo) of row and column strips: the seams the states put their features on (a grid without
    a seam gets them in the middle)"""
    qx, qy = nx + 2 * NG, ny + 2 * NG
    seed = state_seed(nx, ny, kind)
    rng = np.random.default_rng(seed + 1)
    rho, u, v, p = smooth_prims(nx, ny, seed)
    rows = list(rows) or [nx // 2]
    cols = list(cols) or [ny // 2]
    if kind == "smooth":
        return cons(rho, u, v, p)
    if kind == "super":
        # |u|, |v| of 2.5 (c is about 1 .. 1.4), the signs changing at the first row / column seam
        u = u + np.where(np.arange(qx)[:, None] < NG + rows[0], 2.5, -2.5)
        v = v + np.where(np.arange(qy)[None, :] < NG + cols[0], -2.5, 2.5)
        return cons(rho, u, v, p)
    if kind == "zeros":
        # blocks of +0 / -0 momenta that straddle every row seam (all columns of a band around a
        # column seam) and every column seam (all rows of a band around a row seam), next to moving gas
        U = cons(rho, u, v, p)
        for n, r in enumerate(rows):
            i0, i1 = max(NG + r - 3, 0), NG + r + 3
            for m, c in enumerate(cols):
                j0, j1 = max(NG + c - 3, 0), NG + c + 3
                for var in (2, 3):
                    z = 0.0 if (n + m + var) % 2 else -0.0
                    U[i0:i1, j0:j1, var] = np.where(rng.random(U[i0:i1, j0:j1, var].shape) < 0.8, z, -z)
                U[i0:i1, j0:j1, 1] = p[i0:i1, j0:j1] / (GAMMA - 1.0)
        return U
    if kind == "sedov":
        # the reference's Sedov set-up in strength (ambient e = 1e-6 / (gamma - 1), density 1, gas at
        # rest; the hot region's energy 10): the hot region is the corner block below the last row
        # seam and the last column seam, so that the front lies on a seam in both directions
        rho = 1.0 + 0.0 * rho
        E = np.full((qx, qy), 1.e-6 / (GAMMA - 1.0))
        E[:NG + rows[-1], :NG + cols[-1]] = 10.0
        z = np.zeros((qx, qy))
        return np.ascontiguousarray(np.stack([rho, E, z, z], axis=-1))
    if kind in ("floor", "floor_wall"):
        # densities of 0.2 SMALL_DENS in interior cells on either side of every seam, and in two
        # cells of the first and last column: clean_state floors them.  None of them in the first or
        # the last row: beside an oddly reflecting boundary (the Sedov set-up's reflect-odd: the ghost
        # density is MINUS the cell's, not floored) the slope of such a cell makes the density of the
        # face state at the boundary negative, and there the reference's two-shock solver returns
        # cancellation noise times 1e20 (c floored at smallc = 1e-10, riemann.py:88-101): its own
        # answer moves by 1e-2 when the input moves by an ulp -- `floor_wall`, which has such a cell,
        # and test_sph_oracle.py::test_oracle_floor_beside_odd_wall_turns_on_an_ulp show it
        rho = rho.copy()
        inner = lambda n: 1 + n % (nx - 2)         # a row in 1 .. nx - 2
        for r in rows:
            for d in (-1, 0):
                if 1 <= r + d <= nx - 2:
                    rho[NG + r + d, NG + (3 * r + d) % ny] = 0.2 * SMALL_DENS
        for c in cols:
            for d in (-1, 0):
                if 0 <= c + d < ny:
                    rho[NG + inner(5 * c + d), NG + c + d] = 0.2 * SMALL_DENS
        rho[NG + 1, NG] = rho[NG + nx - 2, NG + ny - 1] = 0.2 * SMALL_DENS
        if kind == "floor_wall":
            rho[NG, NG + 2] = 0.2 * SMALL_DENS
        return cons(rho, u, v, p)
    raise ValueError(kind)
