"""Shapes and states for the shallow-water kernels against the C oracle (tests/test_swe_oracle.py;
tests/test_fastseed_emu.py takes the `blocks` state from here).

Shapes: one for every path of k_sw_wave's unit decoding (csrc/swe.hip: sww_geometry), for 4
compute units (the emulated device) and 256 (the MI355X) -- PATHS names them and
test_swe_oracle.py::test_wave_geometry_reaches_every_path holds the list to the library's own
geometry call -- and the column counts around the 58 updated columns of a wavefront and around
the staged kernels' 256-thread blocks.

States (qx, qy, 4) over the WHOLE array: the ghost cells hold arbitrary valid values, not
boundary-consistent ones.  All seeded."""
import numpy as np

NG = 4
SWW_OUT = 58          # columns a wavefront of k_sw_wave updates

# (nx, ny): dy / dx and g alternate between (1.3, 1.0) and (0.7, 2.0) down the list
SHAPES = [(5, 7), (9, 300), (17, 61), (23, 59), (40, 130), (64, 400), (21, 117), (18, 57), (19, 58),
          (20, 116), (6, 254), (7, 255), (8, 257)]
BIG = (816, 2320)     # cut and regular column strips side by side on 256 compute units (GPU only)
PARAMS = [(1.3, 1.0), (0.7, 2.0)]       # (dy / dx, g)

# path of the unit decoding -> {compute units: shapes that must take it}
PATHS = {
    "single_chunk": {4: [(5, 7), (9, 300)], 256: [(5, 7), (9, 300)]},
    "two_regular_last_1": {4: [(17, 61)], 256: [(17, 61)]},
    "two_regular_last_7": {4: [(23, 59)], 256: [(23, 59)]},
    "all_cut": {4: [(40, 130)], 256: [(40, 130)]},
    "cut_and_regular": {4: [(64, 400)], 256: [BIG]},
}


STATES = ("smooth", "super", "zeros", "dry", "blocks")
SOLVERS = ("Roe", "HLLC")
LIMITERS = (0, 1, 2)
LARGE = ((64, 400), BIG)
# seed multiplier k of the `blocks` state per shape (state_seed: 1000 k + 7 nx + ny; default 1): the
# FIRST k >= 1 for which the oracle's step is finite on every case in_finite_list() keeps for the
# shape and, with HLLC and limiter 0, has faces of negative height in both directions.  The oracle
# alone decides, no kernel.  After a change of make_state, of row_seams or of the library's row
# strips (sww_rows moves the seams), test_swe_oracle.py::test_case_list_conditions says which
# shape needs the search again: run its loop over k = 1, 2, ... for that shape.
BLOCK_SEED = {(23, 59): 3, (18, 57): 2, (20, 116): 2, (6, 254): 2, (64, 400): 2}


def in_finite_list(shape, kind, riemann, limiter):
    """the cases on which the reference's own step is finite (the oracle confirms it:
    test_swe_oracle.py::test_case_list_conditions).  Left out, as states on which the reference
    itself returns NaN:
    - Roe with limiter 0 on `blocks` and `dry`: the unlimited slopes give negative face heights,
      and riemann_roe takes sqrt(h_l), sqrt(h_r) (interface.py:290-300);
    - Roe on `blocks` on the two large shapes: piecewise-constant data hands riemann_roe left
      and right states that are equal to the bit, where its Harten-Hyman fix is
      lambda * 0 / 0 as soon as a wave speed is within its tol = 0.01 of zero (interface.py:
      353-362); among the thousands of blocks of these shapes some always are;
    - HLLC with limiter 0 on `blocks` at 816 x 2320: the same count of blocks, 0 / 0 in S_c
      between two faces of negative height."""
    if riemann == "Roe" and limiter == 0 and kind in ("blocks", "dry"):
        return False
    if riemann == "Roe" and kind == "blocks" and tuple(shape) in LARGE:
        return False
    if tuple(shape) == BIG and kind == "blocks" and limiter == 0:
        return False
    return True


def state_seed(shape, kind):
    nx, ny = shape
    return 1000 * (BLOCK_SEED.get(tuple(shape), 1) if kind == "blocks" else 1) + nx * 7 + ny


def shape_params(shape):
    """(dx, dy, g) of a shape of SHAPES / BIG"""
    aspect, g = PARAMS[(SHAPES.index(shape) if shape in SHAPES else 0) % 2]
    dx = 1.0 / 64
    return dx, aspect * dx, g


def path_of(geo, nx):
    """which path of k_sw_wave's unit decoding a geometry (device.swe_wave_geometry) takes, and
    the rows [i0, i1) of every row strip in it, as offsets from ilo: (name, regular, cut)"""
    L, nsb, ne, ncb = geo["rows_per_strip"], geo["row_strips"], geo["n_extra"], geo["col_strips"]
    regular = [(sb * L, min(sb * L + L, nx)) for sb in range(nsb)]
    cut = [(sb * nx // (nsb + 1), (sb + 1) * nx // (nsb + 1)) for sb in range(nsb + 1)]
    if ne == 0:
        if nsb == 1:
            return "single_chunk", regular, []
        if nsb == 2:
            return f"two_regular_last_{regular[-1][1] - regular[-1][0]}", regular, []
        return "regular", regular, []
    return ("all_cut", [], cut) if ne == ncb else ("cut_and_regular", regular, cut)


def row_seams(nx, geos):
    """first rows (offsets from ilo) of the row strips of the given geometries"""
    out = set()
    for geo in geos:
        _, regular, cut = path_of(geo, nx)
        out |= {a for a, _ in regular + cut if 0 < a < nx}
    return sorted(out)


def smooth_state(nx, ny, seed):
    """the smooth random state of tests/test_swe.py"""
    ng = NG
    rng = np.random.default_rng(seed)
    x = np.arange(nx + 2 * ng)[:, None] / nx
    y = np.arange(ny + 2 * ng)[None, :] / ny
    U0 = np.zeros((nx + 2 * ng, ny + 2 * ng, 4))
    U0[..., 0] = 1.0 + 0.3 * np.sin(6 * x) * np.cos(4 * y) + 0.05 * rng.random(U0.shape[:2])
    U0[..., 1] = U0[..., 0] * (0.4 * np.cos(3 * x + y))
    U0[..., 2] = U0[..., 0] * (-0.5 * np.sin(5 * y - x))
    U0[..., 3] = U0[..., 0] * (0.5 + 0.5 * np.sin(9 * x * y))
    return U0


# (h, u, v, X) of the blocks: heights 0.25 .. 4 (ratios up to 16), both signs of every velocity,
# sub- and supercritical; no block is exactly critical (|u| = sqrt(g h) for g = 1 or 2)
BLOCK_STATES = np.array([[1.0, 0.0, 0.0, 1.0], [0.25, 0.3, -0.2, 0.1], [4.0, -0.5, 0.4, 0.7],
                         [0.5, 2.5, -2.5, 0.3], [2.0, -3.0, 3.0, 0.9], [0.25, -0.1, 0.2, 0.5],
                         [4.0, 0.7, -0.6, 0.2], [1.5, 0.2, 1.9, 0.6]])


def make_state(kind, nx, ny, g, seed, seams=()):
    """a state (qx, qy, 4) of the given kind; seams: first rows (offsets from ilo) of row strips
    for `blocks` to put jumps on"""
    ng = NG
    qx, qy = nx + 2 * ng, ny + 2 * ng
    rng = np.random.default_rng(seed)
    U = smooth_state(nx, ny, seed)
    if kind == "smooth":
        return U
    h = U[..., 0].copy()
    u, v, X = (U[..., n] / h for n in (1, 2, 3))
    if kind == "super":
        # |u|, |v| of 2.5 (c is about 1 .. 1.6) with opposite signs in the two halves
        u = u + np.where(np.arange(qx)[:, None] < qx // 2, 2.5, -2.5)
        v = v + np.where(np.arange(qy)[None, :] < qy // 2, -2.5, 2.5)
        return np.ascontiguousarray(np.stack([h, h * u, h * v, h * X], axis=-1))
    if kind == "dry":
        dry = rng.random((qx, qy)) < 0.05
        dry[ng, ng] = dry[ng + nx - 1, ng + ny - 1] = dry[1, 2] = True
        h = np.where(dry, 1e-8, h)
        return np.ascontiguousarray(np.stack([h, h * u, h * v, h * X], axis=-1))
    if kind == "zeros":
        # patches of +0 and -0 in the conserved momenta, next to moving water; single cells at
        # exactly |u| = c (e_val[0] = u - c = +0, e_val[2] = u + c = +0; never a uniform block of
        # them); and a band of still water over all rows, 25 columns wide where the grid has them,
        # with seeded signs of its zeros: its middle stays at rest for three steps, so that a
        # final state has exact zeros whose signs can be compared
        U = np.ascontiguousarray(np.stack([h, h * u, h * v, h * X], axis=-1))
        for n_patch in range(max(4, nx * ny // 150)):
            i, j = rng.integers(0, qx - 2), rng.integers(0, qy - 2)
            U[i:i + 3, j:j + 3, 1 + n_patch % 2] = 0.0 if (n_patch // 2) % 2 else -0.0
        for n_c in range(4):
            i, j = ng + 1 + rng.integers(0, nx - 2), ng + 1 + rng.integers(0, ny - 2)
            U[i, j, 0] = 1.0 / g
            U[i, j, 1 + n_c % 2] = (1.0 if n_c < 2 else -1.0) / g
        if ny >= 40:
            w = 25
            j0 = ng + (ny - w) // 2
            U[:, j0:j0 + w, 0] = 1.25
            for n in (1, 2):
                U[:, j0:j0 + w, n] = np.where(rng.random((qx, w)) < 0.5, 0.0, -0.0)
            U[:, j0:j0 + w, 3] = 0.5
        return U
    if kind == "blocks":
        # piecewise-constant blocks of 3 x 3 cells, with further jumps on and next to the seams of the
        # column strips (j = jlo + 58 m + {-1, 0, 1}) and of the row strips (i = ilo + seam + {-1, 0, 1})
        cx = {i for i in range(ng, qx, 3)} | {ng + s + d for s in seams for d in (-1, 0, 1)}
        cy = {j for j in range(ng, qy, 3)} | {ng + SWW_OUT * m + d for m in range(ny // SWW_OUT + 2) for d in (-1, 0, 1)}
        cx, cy = sorted(c for c in cx if 0 < c < qx), sorted(c for c in cy if 0 < c < qy)
        bi = np.searchsorted(cx, np.arange(qx), side="right")
        bj = np.searchsorted(cy, np.arange(qy), side="right")
        pick = rng.integers(0, len(BLOCK_STATES), size=(len(cx) + 1, len(cy) + 1))
        S = BLOCK_STATES[pick[bi][:, bj]]
        h, u, v, X = (S[..., n] for n in range(4))
        return np.ascontiguousarray(np.stack([h, h * u, h * v, h * X], axis=-1))
    if kind == "critical":
        # the NaN-pattern case: a uniform, exactly critical block (u = sqrt(g h) to the bit) inside the
        # smooth state -- the reference's Harten-Hyman fix is 0 * x / 0 there
        i0, j0 = ng + nx // 3, ng + ny // 3
        U[i0:i0 + 6, j0:j0 + 6] = [1.0 / g, 1.0 / g, 0.0, 0.5 / g]
        return U
    raise ValueError(kind)
