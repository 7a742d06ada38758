"""Shapes, states and parameters for the Cartesian CTU step kernels against the C oracle
(tests/test_ctu_oracle.py): the staged set, the tile kernel k_ctu_fused (csrc/comp_fused.hip) and
the row-marching kernel k_ctu_wave (csrc/comp_wave.hip).

Shapes: one for every path of k_ctu_wave's unit decoding, for 4 compute units (the emulated device)
and 256 (the MI355X) -- PATHS names them, and test_ctu_oracle.py::test_wave_plan_reaches_every_path
holds the list to the library's own plan (device.comp_wave_plan: the function the step goes by).
Column counts lie around 1, 2 and 3 times the 56 updated columns of a wavefront and around 30 / 60 /
90, the interior of the tile kernel's 14 x 30 tiles; row counts around 8 (the library's shortest
strip), 14 / 28 (the tiles), 32 (from where the library cuts row strips).  Where a path depends on
the number of wavefront slots its shape is searched through the plan (pick_*), never written down.

States: sph_cases.make_state (a Cartesian state has the same four planes), features on the seams of
both devices' strips and of the tiles.  Two things are kept out of the list, each for a reason that an
oracle-only test of test_ctu_oracle.py shows: gravity over the `sedov` state (a cold gas at rest) and
supersonic gas running INTO a y side (make_state below turns the `super` state's y momentum round)."""
import functools

import sph_cases as sc
from sph_cases import CFL, GAMMA, GRAV, NG, SMALL_DENS, STATES, solid  # noqa: F401

WOUT = 56             # columns a wavefront of k_ctu_wave updates
TILE = (14, 30)       # cells a workgroup of k_ctu_fused updates (fused_common.h: FTI x FTJ)
DOMAIN = (1.0, 1.5)   # xmax, ymax (xmin = ymin = 0): dx = 1 / nx, dy = 1.5 / ny

# (nx, ny, march_rows): at most 1e4 cells each
SHAPES = [(4, 4, 0), (8, 57, 0), (31, 55, 0), (32, 56, 0),
          (33, 112, 0), (35, 113, 0), (36, 60, 11), (33, 56, 5),
          (70, 57, 11),
          (5, 57, 1), (12, 113, 3), (66, 4, 11),
          (40, 169, 0), (70, 120, 0),
          (70, 58, 1),
          (14, 30, 0), (15, 31, 0), (29, 61, 0), (43, 91, 0)]
# searched shapes (pick): name -> what the search looks for
PICKED = ("allcut", "mixed", "short", "noprio")
SHORT_MARCH = 16      # rows per strip of the short-tail shapes: the shortest strip wave_short_tail cuts
NOPRIO_NX = 70


def make_state(kind, nx, ny, rows=(), cols=()):
    """sph_cases.make_state, the `super` state with its y momentum reversed: the gas runs at Mach 2
    TOWARDS the first column seam from both sides (a collision ON the seam) and away from the y sides.
    Running into a reflecting y side it meets its own mirror image, and the reference's two-shock solver
    has a branch of its own for u* == 0 exactly: an ulp decides there
    (test_oracle_cgf_wall_collision_turns_on_an_ulp)"""
    U = sc.make_state(kind, nx, ny, rows, cols)
    if kind == "super":
        U[..., 3] = -U[..., 3]
    return U


def _search(plan, cus, march_rows, want, col_strips, rows_of):
    """the shape (nx, 56 ncb - 3, march_rows) of the fewest cells -- the squarest among equals --
    whose plan on `cus` compute units satisfies `want`; rows_of(ncb): the row counts to try"""
    best = None
    for ncb in col_strips:
        ny = WOUT * ncb - 3
        for nx in rows_of(ncb):
            if best is not None and (nx * ny, max(nx, ny)) >= best[0]:
                continue
            if want(plan(nx, ny, cus, march_rows)):
                best = ((nx * ny, max(nx, ny)), (nx, ny, march_rows))
    assert best is not None, "no such shape"
    return best[1]


def pick(plan, name, cus):
    """the searched shape `name` for `cus` compute units; plan(nx, ny, cus, march_rows) -> dict of
    device.comp_wave_plan"""
    slots = plan(8, 8, cus, 0)["slots"]
    if name == "allcut":      # every column strip cut into row_strips + 1 parts: a launch of one round
        # (the library takes 8-row strips while they fit the slots: the rows around 8 slots / ncb and up)
        return _search(plan, cus, 0, lambda g: g["n_extra"] == g["col_strips"] and g["n_short"] == 0,
                       range(2, 9), lambda ncb: range(max(33, 8 * slots // ncb - 16), 10 * slots // ncb + 24))
    if name == "mixed":       # at least two cut and two regular column strips in one launch
        return _search(plan, cus, 0, lambda g: 2 <= g["n_extra"] <= g["col_strips"] - 2,
                       range(4, 12), lambda ncb: range(max(33, 8 * slots // ncb - 16), 10 * slots // ncb + 24))
    if name == "short":       # many rounds: short row strips end the grid
        cols = [n for n in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048) if n <= slots]
        # (at least two short strips: the second one's first row is not the short region's)
        return _search(plan, cus, SHORT_MARCH, lambda g: g["n_short"] >= 2, cols,
                       lambda ncb: range(SHORT_MARCH * (4 * slots // ncb) - 12, SHORT_MARCH * (4 * slots // ncb + 1) + 1))
    if name == "noprio":      # 1-row strips, more wavefronts than two rounds of slots
        return _search(plan, cus, 1, lambda g: g["prio_duty"] == 0, range(1, 8 * cus),
                       lambda ncb: (NOPRIO_NX,))
    raise ValueError(name)


# path of the unit decoding -> {compute units: shapes that must take it}; a name of PICKED stands for
# pick(plan, name, cus) (on 256 compute units those are large: GPU only)
_BOTH = lambda shapes: {cus: list(shapes) for cus in (4, 256)}        # noqa: E731
PATHS = {
    "one_strip": _BOTH([(4, 4, 0), (8, 57, 0), (31, 55, 0), (32, 56, 0), (14, 30, 0), (15, 31, 0), (29, 61, 0)]),
    "joined_last": _BOTH([(33, 112, 0), (35, 113, 0), (36, 60, 11), (33, 56, 5), (43, 91, 0)]),
    "last_ng": _BOTH([(70, 57, 11)]),
    "march_rows": _BOTH([(36, 60, 11), (33, 56, 5), (70, 57, 11), (5, 57, 1), (12, 113, 3), (66, 4, 11), (70, 58, 1)]),
    "one_row_strips": _BOTH([(5, 57, 1), (70, 58, 1)]),
    "regular_strips": _BOTH([(40, 169, 0), (70, 120, 0)]),
    "all_cut": {4: ["allcut"], 256: ["allcut"]},
    "cut_and_regular": {4: ["mixed"], 256: ["mixed"]},
    "short_tail": {4: ["short"], 256: ["short"]},
    "no_priority": {4: [(70, 58, 1), "short"], 256: ["noprio", "short"]},
}


def strips_of(g, nx):
    """rows [i0, i1) (offsets from ilo) of the row strips of a plan (device.comp_wave_plan):
    (regular, cut) -- regular: long_row_strips of L rows, then n_short of short_rows, the last one to
    the end (it holds a joined short tail); cut: the row_strips + 1 equal parts of the column strips
    [0, n_extra)"""
    L, nsb, ne, ns, Ls, nl = (g[k] for k in ("rows_per_strip", "row_strips", "n_extra", "n_short",
                                             "short_rows", "long_row_strips"))
    if ns == 0:
        starts = [sb * L for sb in range(nsb)]
    else:
        starts = [sb * L for sb in range(nl)] + [nl * L + k * Ls for k in range(ns)]
    regular = [(a, b) for a, b in zip(starts, starts[1:] + [nx])]
    cut = [(sb * nx // (nsb + 1), (sb + 1) * nx // (nsb + 1)) for sb in range(nsb + 1)] if ne else []
    return regular, cut


def paths_of(g, nx, march_rows):
    """the names of PATHS a plan takes"""
    L, nsb, ne, ncb = g["rows_per_strip"], g["row_strips"], g["n_extra"], g["col_strips"]
    regular, _ = strips_of(g, nx)
    last = regular[-1][1] - regular[-1][0]
    out = set()
    if g["n_short"] > 0:
        out.add("short_tail")
    elif ne == 0:
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
        if march_rows == 0 and nsb > 1 and last <= L:
            out.add("regular_strips")
    else:
        out.add("all_cut" if ne == ncb else "cut_and_regular")
    if g["prio_duty"] == 0:
        out.add("no_priority")
    return out


def row_seams(nx, plans):
    """first rows (offsets from ilo) of the row strips of the given plans, and of the tile kernel's tiles"""
    out = set(range(TILE[0], nx, TILE[0]))
    for g in plans:
        regular, cut = strips_of(g, nx)
        out |= {a for a, _ in regular + cut if 0 < a < nx}
    return sorted(out)


def col_seams(ny):
    """first columns (offsets from jlo) of the column strips behind the first, and of the tiles"""
    return sorted(set(range(WOUT, ny, WOUT)) | set(range(TILE[1], ny, TILE[1])))


# ---------------------------------------------------------------- parameters
BCS = [("outflow", "outflow", "outflow", "outflow"),
       ("reflect", "outflow", "periodic", "periodic"),
       ("reflect", "reflect", "reflect", "reflect"),
       ("periodic", "periodic", "reflect", "outflow")]
SOLVERS = ("HLLC", "CGF", "HLLC_lm")
# (limiter, use_flattening, grav): every value of each, both template instances STD (limiter 2 with
# flattening) and not, each with and without gravity
PARAMS = [(2, 1, 0.0), (2, 1, GRAV), (0, 1, 0.0), (1, 0, GRAV), (2, 0, 0.0), (0, 0, GRAV), (1, 1, GRAV)]


def cases_of(shape, n_shape):
    """the cases of a shape: every state; the boundary mixes, the solvers and the parameter rows taken
    in turn (the offsets move with the shape's place in the list, so that over the list every state
    meets every boundary mix and every solver, and every parameter row every kind of shape):
    (state, bcs, limiter, use_flattening, grav, solver, small_dens).  A shape of more than 3e4 cells (the
    short-tail shape of the emulated device: a hundred thousand) takes ONE state, its turn in the list"""
    out = []
    for n, kind in enumerate(STATES):
        if shape[0] * shape[1] > 3e4 and n != n_shape % len(STATES):
            continue
        lim, flat, grav = PARAMS[(n_shape * 3 + n) % len(PARAMS)]
        if kind == "sedov":       # (test_oracle_cold_gas_at_rest_turns_on_the_sign_of_a_zero)
            grav = 0.0
        out.append((kind, BCS[(n_shape + n) % len(BCS)], lim, flat, grav, SOLVERS[(n_shape + 2 * n) % 3],
                    SMALL_DENS if kind == "floor" else -1.e200))
    return out


@functools.lru_cache(maxsize=None)
def spacing(nx, ny):
    return DOMAIN[0] / nx, DOMAIN[1] / ny


assert sc.SWOUT == WOUT
