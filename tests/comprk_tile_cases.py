"""Cases of tests/test_comprk_tile.py: grid shapes on the seams of the compressible_rk stage tile
kernel (k_rk_tile, csrc/comp_rk_tile.hip), the covering list of methods / solvers / reconstructions /
boundaries, and the states.  Shapes are functions of the tile (TX, TY) that
pyrohip_comp_rk_tile_geometry reports, so a change of the tile moves them along."""
import numpy as np

NG = 4
GAMMA = 1.4
CFL = 0.8
SMALL_DENS = 0.35            # the floor of the "floor" state (its thin cells lie below it)

METHODS = ("RK2", "TVD2", "TVD3", "RK4")
RIEMANN = ("HLLC", "CGF", "HLLC_lm")
LIMITERS = (0, 1, 2)
FLATTEN = (0, 1)
GRAVS = (0.0, -1.0)
BC_MIXES = {
    "outflow": ("outflow", "outflow", "outflow", "outflow"),
    "reflect": ("reflect", "reflect", "reflect", "reflect"),        # odd normal momentum (orc.comp_var_bcs)
    "periodic": ("periodic", "periodic", "periodic", "periodic"),
    "outflow-x/periodic-y": ("outflow", "outflow", "periodic", "periodic"),
    "reflect-x/periodic-y": ("reflect", "reflect", "periodic", "periodic"),
}
STATES = ("smooth", "jump", "zeros", "floor")


def shapes(tx, ty):
    """the shapes every run of the suite takes, by the kernel's tile"""
    return [(4, 4), (4, ty + 1), (tx + 1, 4), (tx, ty), (tx + 1, ty + 1), (2 * tx - 1, 2 * ty + 1),
            (5, 3 * ty + 2)]


def gpu_shapes(tx, ty):
    """... and on the GPU alone: 8 x 8 tiles, two ragged many-tile grids"""
    return [(8 * tx, 8 * ty), (127, 250), (1021, 67)]


def case_list(nshapes=7, per_shape=6):
    """(shape index, method, riemann, limiter, flattening, grav, boundary mix, state): a covering
    list, not the full product -- covers() holds it to "every value at three shapes or more" """
    mixes = list(BC_MIXES)
    out = []
    for si in range(nshapes):
        for r in range(per_shape):
            c = si * per_shape + r
            st, lim = STATES[(c + 3 * si) % 4], LIMITERS[(c // 2 + si) % 3]
            # The jump meets the limited reconstructions only.  Unlimited centred slopes across a
            # pressure jump of 10^3 in slowly moving gas (no compression that would switch the flattening
            # on) put the low side's face pressure near p - 250 p: a face state that is no gas.  What a
            # Riemann solver makes of the roots of negative numbers is its arithmetic's own; the
            # contracted build is held to 1e-10 of the bit-faithful one on gas, as everywhere in this
            # suite (test_comp_wave_oddly_reflected_density says the same of the row-marching kernel).
            if st == "jump" and lim == 0:
                lim = 1 + c % 2
            out.append((si, METHODS[(c + si) % 4], RIEMANN[(c + si // 3) % 3], lim,
                        FLATTEN[(c + si) % 2], GRAVS[(c // 3 + si) % 2], mixes[(c + 2 * si) % 5], st))
    return out


def covers(cases):
    """every value of every parameter appears at three different shapes or more"""
    for col, values in ((1, METHODS), (2, RIEMANN), (3, LIMITERS), (4, FLATTEN), (5, GRAVS),
                        (6, tuple(BC_MIXES)), (7, STATES)):
        for v in values:
            if len({c[0] for c in cases if c[col] == v}) < 3:
                return False, (col, v)
    return True, None


def _cons(rho, u, v, p):
    return np.stack([rho, p / (GAMMA - 1.0) + 0.5 * rho * (u * u + v * v), rho * u, rho * v], axis=-1)


def seam(n, t):
    """first interior cell behind the first tile seam along a direction of n cells and tiles of t
    (the middle of a grid that has no seam)"""
    return t if n > t else n // 2


def state(kind, nx, ny, tx, ty, seed=0):
    """the whole array (ghost cells hold what the formulas give: every path fills them first)"""
    qx, qy = nx + 2 * NG, ny + 2 * NG
    rng = np.random.default_rng(1000 * nx + ny + seed)
    x = ((np.arange(qx) - NG + 0.5) / nx)[:, None] * np.ones((1, qy))
    y = ((np.arange(qy) - NG + 0.5) / ny)[None, :] * np.ones((qx, 1))
    rho = 1.0 + 0.3 * np.sin(5 * x) * np.cos(3 * y) + 0.05 * rng.random((qx, qy))
    u = 0.3 * np.cos(4 * x + y)
    v = -0.2 * np.sin(3 * y - 2 * x)
    p = 1.0 + 0.5 * np.cos(2 * x) * np.sin(2 * y)
    si, sj = NG + seam(nx, tx), NG + seam(ny, ty)
    if kind == "jump":        # an energy jump of 10^3 whose edges lie on the tile seams
        p = np.where((np.arange(qx)[:, None] < si) & (np.arange(qy)[None, :] < sj), 1.0e3 * p, p)
    elif kind == "zeros":     # gas at rest in x in bands of +0 / -0, at rest in y beside the seam
        u = np.where((np.arange(qx) % 4 < 2)[:, None], -0.0, 0.0) * np.ones((1, qy))
        v = np.where((np.arange(qy)[None, :] >= sj - 1) & (np.arange(qy)[None, :] <= sj), -0.0, v)
    elif kind == "floor":     # cells below small_dens: one on the seam corner, one in a tile, one at the border
        for (i, j) in ((si, sj), (si - 1, sj - 1), (NG, NG + ny - 1), (NG + nx // 2, NG + 1)):
            rho[i, j] = 0.2
    U = _cons(rho, u, v, p)
    if kind == "zeros":
        assert np.signbit(U[..., 2]).any() and not np.signbit(U[..., 2]).all()
    return np.ascontiguousarray(U)
