"""The Cartesian CTU step kernels -- the staged set, the one-launch tile kernel k_ctu_fused
(csrc/comp_fused.hip) and the row-marching kernel k_ctu_wave (csrc/comp_wave.hip) in its bit-faithful
and contracted builds, the device-side stepping loop on top of it -- against the C oracle
orc.comp_step (oracle/pyro_oracle.c, pinned to the reference by tests/test_oracle_golden.py) at the
seams of k_ctu_wave's launch plan and of the tile kernel's tiles.

Shapes, states and parameters: tests/ctu_cases.py.  Every path of the kernel's unit decoding is
reached for 4 compute units (the emulated device) and for 256 (the MI355X); the list is held to the
library's own plan (device.comp_wave_plan: the function the step goes by), so a change of
wave_strip_rows, wave_fill_extra or wave_short_tail that drops a path fails without a launch.

The `dev` tests run on the emulated build here (bit for bit) and on the MI355X under -m gpu."""
import functools

import numpy as np
import pytest

import ctu_cases as cc
from conftest import comp_floors, elementwise_err, max_rel_err
from helpers import DtPolicy
from oracle import orc
from test_device_compressible import TOL_EXACT, TOL_FAST, comp_state

NG = cc.NG
I = (slice(NG, -NG), slice(NG, -NG))
# the searched shapes of the emulated device's 4 compute units, as (name of ctu_cases.PICKED, compute units).
# They are `dev` shapes ABOVE the 1e4 cells of the fixed ones -- 13 860, 15 512 and 103 588 cells -- because the
# cut strips and the short tail exist on no smaller grid of that device (the search returns the smallest)
PICKED4 = [("allcut", 4), ("mixed", 4), ("short", 4)]
SHAPE_IDS = [f"{a}x{b}m{m}" for a, b, m in cc.SHAPES] + [f"{n}{c}" for n, c in PICKED4]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def plan(nx, ny, cus, march_rows, neighbours=False):
    from pyro2_amd import device
    return device.comp_wave_plan(nx, ny, NG, cus, march_rows, neighbours)


@functools.lru_cache(maxsize=None)
def resolve(shape, cus=4):
    """a shape as it is; a name of ctu_cases.PICKED searched for `cus` compute units; (name, cus)"""
    if isinstance(shape, str):
        return cc.pick(plan, shape, cus)
    if isinstance(shape[0], str):
        return cc.pick(plan, *shape)
    return shape


def shape_list():
    return list(cc.SHAPES) + PICKED4


@functools.lru_cache(maxsize=None)
def seams(shape):
    """row and column seams of a shape: of the strips of both devices, and of the tiles"""
    nx, ny, mr = shape
    return tuple(cc.row_seams(nx, [plan(nx, ny, cus, mr) for cus in (4, 256)])), tuple(cc.col_seams(ny))


def oracle_params(shape, case):
    nx, ny, _ = shape
    kind, bcs, lim, flat, grav, solver, sd = case
    dx, dy = cc.spacing(nx, ny)
    return orc.comp_params(nx, ny, NG, dx, dy, gamma=cc.GAMMA, limiter=lim, use_flattening=flat,
                           grav=grav, small_dens=sd, bcs=tuple(bcs), riemann=solver)


def oracle_fill(U, shape, case):
    nx, ny, _ = shape
    return orc.comp_fill_bc(U, nx, ny, NG, list(case[1]), cc.GAMMA, case[4], cc.spacing(nx, ny)[1])


@functools.lru_cache(maxsize=None)
def oracle_case(shape, case):
    """one oracle step of a case, computed once and shared (read-only): (filled input, result, dt, rc)"""
    nx, ny, _ = shape
    dx, dy = cc.spacing(nx, ny)
    rows, cols = seams(shape)
    U0 = oracle_fill(cc.make_state(case[0], nx, ny, rows, cols), shape, case)
    dt = orc.comp_dt(U0, nx, ny, NG, dx, dy, cc.GAMMA, cc.CFL)
    Uo = U0.copy()
    rc, _ = orc.comp_step(Uo, oracle_params(shape, case), dt)
    U0.flags.writeable = Uo.flags.writeable = False
    return U0, Uo, dt, rc


def device_params(shape, case, **kw):
    """solid_xl / solid_yl as orc.comp_params derives them from the sides (the CGF wall rule)"""
    from pyro2_amd import device
    nx, ny, mr = shape
    kind, bcs, lim, flat, grav, solver, sd = case
    dx, dy = cc.spacing(nx, ny)
    Po = oracle_params(shape, case)
    if kw.get("kernel_set") == 2:
        kw.setdefault("march_rows", mr)
    return device.make_comp_params(dx, dy, gamma=cc.GAMMA, limiter=lim, use_flattening=flat, grav=grav,
                                   small_dens=sd, riemann=solver, solid_xl=Po.solid_xl, solid_yl=Po.solid_yl, **kw)


def device_state(dev, shape, case):
    return comp_state(dev, shape[0], shape[1], list(case[1]))


def exact_err(U, Uo):
    """the bit-faithful build's measure in test_device_compressible.py: per variable, over the interior,
    against the variable's largest magnitude (conftest.max_rel_err)"""
    return max(max_rel_err(U[I][..., n], Uo[I][..., n]) for n in range(4))


def fast_err(U, Uo, where=I):
    """the contracted build's: element-wise with that file's floors (conftest.comp_floors)"""
    fl = comp_floors(Uo[where], cc.GAMMA)
    return max(elementwise_err(U[where][..., n], Uo[where][..., n], fl[n]) for n in range(4))


def profiled_step(dev, s, P, dt):
    dev.prof_enable(True)
    dev.prof_report()
    try:
        s.comp_step(P, dt)
        return dev.prof_report()
    finally:
        dev.prof_enable(False)


def wave_alone(rep, slab=False):
    """k_ctu_wave launched once and nothing of the other sets (a slab: its boundary strips may go first
    in a launch of their own -- they do where the backend can overlap them with a halo exchange)"""
    return rep.get("k_ctu_wave", (0, 0))[0] == 1 and rep.get("k_ctu_wave_boundary", (0, 0))[0] <= int(slab) and \
        not any(k in rep for k in ("k_prim", "k_xi", "k_states", "k_ctu_fused"))


# ---------------------------------------------------------------- the case list itself
def test_wave_plan_reaches_every_path(dev):
    """no launch: the shapes of ctu_cases.PATHS take the paths they are listed under, for 4 and for
    256 compute units, by the plan the step itself goes by (pyrohip_comp_wave_plan); the plan is
    consistent in itself and with pyrohip_comp_wave_geometry; every shape of the list stands under a
    path; the column and row counts sit around the strips and tiles they are for; a slab with
    neighbours takes neither cut strips nor a short tail"""
    from pyro2_amd import device
    listed = set()
    for path, by_cus in cc.PATHS.items():
        for cus in (4, 256):
            assert by_cus[cus], (path, cus)
            for name in by_cus[cus]:
                shape = resolve(name, cus)
                nx, ny, mr = shape
                if cus == 4:
                    listed.add(shape)
                    assert shape in [resolve(s) for s in shape_list()], shape
                g = plan(nx, ny, cus, mr)
                regular, cut = cc.strips_of(g, nx)
                assert path in cc.paths_of(g, nx, mr), (path, shape, cus, g)
                ncb, nsb, L, ne = g["col_strips"], g["row_strips"], g["rows_per_strip"], g["n_extra"]
                ns, Ls, nl = g["n_short"], g["short_rows"], g["long_row_strips"]
                geo = device.comp_wave_geometry(nx, ny, NG, cus, mr)
                assert [geo[k] for k in ("col_strips", "rows_per_strip", "row_strips", "overlap", "slots")] == \
                       [g[k] for k in ("col_strips", "rows_per_strip", "row_strips", "overlap", "slots")]
                assert g["slots"] == 8 * cus and ncb == -(-ny // cc.WOUT)
                assert g["wavefronts"] == ncb * (nl + ns) + ne and (nl == nsb if ns == 0 else nl < nsb)
                assert g["prio_duty"] == (0 if g["wavefronts"] > 2 * g["slots"] else 7 if L >= 64 else 6)
                assert regular[0][0] == 0 and regular[-1][1] == nx and len(regular) == nl + ns
                assert all(a[1] == b[0] and a[1] > a[0] for a, b in zip(regular, regular[1:]))
                assert min(b - a for a, b in regular) >= min(NG, nx) or L < NG
                slab = plan(nx, ny, cus, mr, neighbours=True)
                assert slab["n_extra"] == 0 and slab["n_short"] == 0 and slab["wavefronts"] == ncb * nsb
                assert [slab[k] for k in ("col_strips", "rows_per_strip", "row_strips")] == [ncb, L, nsb]
                if path == "one_strip":
                    assert nx <= 32 and nsb == 1 and L == nx and ne == 0
                if path == "joined_last":
                    tail = nx - nsb * L
                    assert 0 < tail < NG and regular[-1] == (nx - L - tail, nx), (shape, g)
                if path == "last_ng":
                    assert nsb >= 2 and regular[-1] == (nx - NG, nx) and L > NG
                if path == "march_rows":
                    assert mr > 0 and L == mr and nsb >= 2 and ne == 0
                if path == "one_row_strips":
                    # (a last strip of one row is shorter than the ghost width: it joins)
                    assert L == 1 and nsb == nx - 1 and regular[-1] == (nx - 2, nx)
                if path == "regular_strips":
                    assert mr == 0 and nsb >= 2 and ne == 0 and ns == 0 and g["wavefronts"] <= g["slots"]
                if path == "all_cut":
                    assert mr == 0 and ne == ncb >= 2 and nsb >= 2 and len(cut) == nsb + 1 and ns == 0
                    assert min(b - a for a, b in cut) >= 8 and cut[0][0] == 0 and cut[-1][1] == nx
                    assert g["wavefronts"] <= g["slots"]
                if path == "cut_and_regular":
                    assert mr == 0 and 2 <= ne <= ncb - 2 and nsb >= 2 and g["wavefronts"] == g["slots"]
                    assert ny % cc.WOUT != 0              # with a ragged last column strip
                if path == "short_tail":
                    assert ns >= 2 and ne == 0 and L >= 16 and Ls == -(-L // (4 if L >= 100 else 2))
                    assert ncb * nsb >= 4 * g["slots"] and regular[nl] == (nl * L, nl * L + Ls)
                    assert regular[nl + 1][0] == nl * L + Ls            # the second short strip
                if path == "no_priority":
                    assert g["wavefronts"] > 2 * g["slots"] and g["prio_duty"] == 0
    assert listed == {resolve(s) for s in shape_list()}, "a shape that stands under no path"
    for shape in cc.SHAPES:                 # every shape stands under a path on both devices
        assert any(shape in by_cus[cus] for by_cus in cc.PATHS.values() for cus in (4, 256)), shape
    # the searched shapes: small on the emulated device, up to a few million cells on 256 compute units
    assert all(np.prod(resolve(n)[:2]) < 1.2e5 for n in PICKED4) and np.prod(resolve(("mixed", 4))[:2]) < 3e4
    assert all(np.prod(resolve(n, 256)[:2]) < 1.2e6 for n in ("allcut", "mixed", "noprio"))
    assert np.prod(resolve("short", 256)[:2]) < 7.5e6         # 8192 units x 16 rows x 56 columns and a bit
    # (every FIXED shape has at most 1e4 cells; the searched ones above do not, see PICKED4 -- and the slab test
    # runs the cut shapes of the device it is on: 0.9 and 1.0 million cells on 256 compute units, no oracle)
    assert all(nx * ny <= 1e4 for nx, ny, _ in cc.SHAPES)
    assert {ny for _, ny, _ in cc.SHAPES} >= {4, 30, 31, 55, 56, 57, 58, 60, 61, 91, 112, 113, 120, 169}
    assert {nx for nx, _, _ in cc.SHAPES} >= {4, 5, 8, 12, 14, 15, 29, 31, 32, 33, 35, 36, 40, 43, 66, 70}
    assert {mr for _, _, mr in cc.SHAPES} == {0, 1, 3, 5, 11}
    # a step that is the only launch of its step takes no short tail: the plan with neighbours = False is the
    # single step's, and comp_evolve(step_launches = 1) is held to the single steps below


def all_cases():
    return [(s, c) for n, s in enumerate(shape_list()) for c in cc.cases_of(resolve(s), n)]


def test_case_list_conditions(dev):
    """the oracle alone, over the whole list, no case left out: rc == 0, every result is finite,
    every step moves the interior by more than 1e-3 of its scale, the `floor` cases have interior
    densities below small_dens and the floor changes their result, the `zeros` cases hold both signs of
    zero; and the list covers every state with every solver and every boundary mix, on single and on
    several column strips, every limiter, flattening on and off, both values of grav (but `sedov`: at
    rest, no gravity), the STD instance (limiter 2 with flattening) and the other one with each solver"""
    seen = set()
    for name, case in all_cases():
        shape = resolve(name)
        kind, bcs, lim, flat, grav, solver, sd = case
        U0, Uo, dt, rc = oracle_case(shape, case)
        tag = (shape, case)
        assert rc == 0 and dt > 0, tag
        assert np.isfinite(Uo).all(), tag
        assert Uo[I][..., 0].min() > 0, tag
        scale = np.abs(U0[I]).max(axis=(0, 1))
        moved = (np.abs(Uo[I] - U0[I]).max(axis=(0, 1)) / np.maximum(scale, 1e-300))
        assert moved[:2].min() > 1e-3 and moved.max() > 1e-3, (tag, moved)
        if kind == "floor":
            assert sd == cc.SMALL_DENS and (U0[I][..., 0] < sd).sum() >= 2, tag
            free = U0.copy()
            unfloored = list(case)
            unfloored[6] = -1.e200
            assert orc.comp_step(free, oracle_params(shape, tuple(unfloored)), dt)[0] == 0
            assert not np.array_equal(free[I], Uo[I]), tag
        else:
            assert U0[I][..., 0].min() > cc.SMALL_DENS
        if kind == "zeros":
            for var in (2, 3):
                z = U0[I][..., var] == 0.0
                assert z.any() and np.signbit(U0[I][..., var][z]).any() and not np.signbit(U0[I][..., var][z]).all(), tag
        multi = shape[1] > cc.WOUT
        std = lim == 2 and flat == 1
        seen |= {("state-bc", kind, bcs), ("state-solver", kind, solver), ("lim", lim), ("flat", flat), ("grav", grav),
                 ("std-solver", std, solver), ("state-cols", kind, multi), ("state-grav", kind, grav), ("std-grav", std, grav)}
    for kind in cc.STATES:
        assert all(("state-bc", kind, b) in seen for b in cc.BCS), kind
        assert all(("state-solver", kind, s) in seen for s in cc.SOLVERS), kind
        assert all(("state-cols", kind, m) in seen for m in (False, True)), kind
        assert all(("state-grav", kind, g) in seen for g in ((0.0,) if kind == "sedov" else (0.0, cc.GRAV))), kind
    assert all(("lim", n) in seen for n in (0, 1, 2)) and all(("flat", n) in seen for n in (0, 1))
    assert all(("std-solver", a, b) in seen for a in (False, True) for b in cc.SOLVERS)
    assert all(("std-grav", a, b) in seen for a in (False, True) for b in (0.0, cc.GRAV))


def test_oracle_cold_gas_at_rest_turns_on_the_sign_of_a_zero(dev):
    """why the `sedov` state is at rest EXACTLY, in the oracle alone: with limiter 0 the unlimited slopes
    at the front (and, under gravity, the predictor's source over the cold gas: E - KE < 0 in every cold
    face state) leave face states that are no gas; HLLC floors both pressures at smallp = 1e-10, the
    contact speed between two such states at rest is (0 + 0 - 0) / ... = 0 exactly, and `S_c <= 0`
    picks the right star state.  An x momentum of +-1e-300 in the cold gas -- far below an ulp of any
    momentum of the problem -- turns that sign and moves the oracle's own answer by more than 0.1:
    no build with another rounding could be held to it.  With exact zeros every build takes the same
    side (0 * anything), and that is what the list holds them to.  Under gravity the list still keeps
    off this state (ctu_cases.cases_of): between two face states that are no gas the contracted HLLC
    (hydro.h: hllc_flux_impl, star) is not the reference's sum -- its collapsed star flux carries the
    FLOORED pressure where the reference's physical flux F_k keeps the raw one, equal for every p >= smallp
    -- and leaves the oracle by 1.45e-3 (limiter 0) and 7.7e-7 (limiter 2, where the oracle does not move:
    DESIGN.md 3.2.1 has the measured price of the missing term;
    test_contracted_hllc_over_cold_gas_under_gravity holds that regime to the bound the missing term allows)"""
    shape = (14, 30, 0)
    nx, ny, _ = shape
    for lim, grav, sensitive in ((0, cc.GRAV, True), (0, 0.0, True), (2, cc.GRAV, False)):
        case = ("sedov", cc.BCS[1], lim, 1, grav, "HLLC", -1.e200)
        U0, Uo, dt, rc = oracle_case(shape, case)
        assert rc == 0 and np.isfinite(Uo).all()
        moves = []
        for eps in (1.e-300, -1.e-300):
            A = np.array(U0)
            A[..., 2] = np.where(A[..., 1] < 1.0, eps, A[..., 2])
            oracle_fill(A, shape, case)
            assert orc.comp_step(A, oracle_params(shape, case), dt)[0] == 0
            moves.append(float(np.abs(A - Uo)[I].max()))
        print(f"limiter {lim} grav {grav}: an x momentum of +-1e-300 moves the oracle by", moves)
        assert (max(moves) > 0.1) if sensitive else (max(moves) < 1e-290), (lim, grav, moves)


# ---------------------------------------------------------------- what the list found
def test_ghost_image_of_a_floored_cell_under_gravity(dev, golden):
    """finding A: the gravity source of a ghost cell that mirrors a FLOORED interior cell.  The reference
    floors the interior in place and leaves the ghost cells as the fill left them, but it fills the
    source's ghost cells from the source's interior (unsplit_fluxes.py:295-306): the ghost image of a
    floored cell carries the floored cell's source.  The recorded step of the reference
    (tests/golden/comp_floor_grav.npz: 8 x 57, periodic in y, floored cells in the first and the last
    column) against all three kernel sets: equal on the emulator (the kernels took the ghost cell's own
    unfloored density: 1.7e-5 off in the cells whose stencil reaches such a ghost cell)"""
    from pyro2_amd import device
    g = golden("comp_floor_grav")
    nx, ny, ng = (int(v) for v in g["grid"])
    gamma, lim, flat, grav, sd, cfl = (float(v) for v in g["params"])
    bcs = [str(b) for b in g["bc"]]
    U0, U1, dt = g["U0"], g["U1"], float(g["dt"])
    Po = orc.comp_params(nx, ny, ng, *g["dxdy"], gamma=gamma, limiter=int(lim), use_flattening=int(flat), grav=grav,
                         small_dens=sd, bcs=tuple(bcs))
    s = comp_state(dev, nx, ny, bcs)
    for ks, fastm in ((0, 0), (1, 0), (2, 0), (1, 1), (2, 1)):
        P = device.make_comp_params(*g["dxdy"], gamma=gamma, limiter=int(lim), use_flattening=int(flat), grav=grav,
                                    small_dens=sd, solid_xl=Po.solid_xl, solid_yl=Po.solid_yl, kernel_set=ks,
                                    fast_math=fastm)
        s.upload(U0)
        s.fill_bc()
        assert np.array_equal(bits(s.download()), bits(U0))
        s.comp_step(P, dt)
        U = s.download()
        err = fast_err(U, U1) if fastm else exact_err(U, U1)
        print(f"kernel_set {ks} fast_math {fastm}: err against the reference's step {err:.3e}")
        if fastm:
            assert err <= TOL_FAST, (ks, err)
        elif dev.kind == "emu":
            assert np.array_equal(U[I], U1[I]), (ks, np.argwhere(U[I] != U1[I])[:8])
        else:
            assert err <= TOL_EXACT, (ks, err)


@pytest.mark.parametrize("lim", [1, 2])
def test_contracted_hllc_over_cold_gas_under_gravity(dev, lim):
    """the regime the list keeps off (finding B), held where the reference is well conditioned: 14 x 30, the
    `sedov` state, HLLC, grav -0.3, limited slopes.  The bit-faithful kernel sets equal the oracle.  The
    contracted HLLC's star flux carries the floored pressure p = max(pf, smallp) where the reference's
    physical flux keeps the raw pf: per face it is off by (pf - p) (0, u, 1, 0) and by nothing else but
    rounding, so a cell moves by at most (2 dt/dx + 2 dt/dy) max (smallp - pf) max(1, |u|) over the face
    states the ORACLE's stages hold (predictor and final ones) -- the bound, 3.3e-7 here, comes from the
    reference's stage data, not from the kernels -- plus TOL_FAST of the cell's scale"""
    shape = (14, 30, 0)
    nx, ny, _ = shape
    dx, dy = cc.spacing(nx, ny)
    case = ("sedov", cc.BCS[1], lim, 1, cc.GRAV, "HLLC", -1.e200)
    U0, Uo, dt, rc = oracle_case(shape, case)
    A = np.array(U0)
    rc, st = orc.comp_step(A, oracle_params(shape, case), dt, stages=True)
    assert rc == 0 and np.array_equal(A, Uo)
    gap, umax = 0.0, 1.0
    for nm in ("Uxl0", "Uxr0", "Uyl0", "Uyr0", "Uxl", "Uxr", "Uyl", "Uyr"):
        F = st[nm][NG - 1:-NG + 2, NG - 1:-NG + 2]
        pf = (cc.GAMMA - 1.0) * (F[..., 1] - 0.5 * (F[..., 2] ** 2 + F[..., 3] ** 2) / F[..., 0])
        gap = max(gap, float((1.e-10 - pf).max()))
        umax = max(umax, float(np.abs(F[..., 2:] / F[..., :1]).max()))
    assert gap > 1.e-7, "the premise: face states with E - KE < 0"
    bound = 2.0 * (dt / dx + dt / dy) * gap * umax
    s = device_state(dev, shape, case)
    for ks, fastm in ((0, 0), (1, 0), (2, 0), (1, 1), (2, 1)):
        s.upload(U0)
        s.fill_bc()
        s.comp_step(device_params(shape, case, kernel_set=ks, fast_math=fastm), dt)
        U = s.download()
        diff = float(np.abs(U - Uo)[I].max())
        print(f"limiter {lim} kernel_set {ks} fast_math {fastm}: max |U - oracle| {diff:.3e} (bound {bound:.3e})")
        if fastm:
            assert (np.abs(U - Uo)[I] <= bound + TOL_FAST * np.abs(Uo[I])).all(), (ks, diff, bound)
        elif dev.kind == "emu":
            assert np.array_equal(U[I], Uo[I]), ks
        else:
            assert exact_err(U, Uo) <= TOL_EXACT, ks


def test_oracle_cgf_wall_collision_turns_on_an_ulp(dev):
    """why the `super` state of this list runs AWAY from the y sides (ctu_cases.make_state), in the oracle
    alone.  Gas that runs into a reflecting side meets its mirror image in the ghost cells: at the wall's
    face W_l u_l + W_r u_r + (p_l - p_r) is 0 to the bit, and u* == 0 exactly is a branch of its own in the
    reference's two-shock solver (riemann.py: the average of the two star states).  With u* a rounding
    residue of either sign the supersonic side's OUTER state is taken instead (sigma > 0).  One ulp more
    y momentum in ONE ghost cell of the filled input moves the oracle's own answer in the cell beside it
    by more than 1e-2 in the contracted build's measure, eight decades above its bar: no build that
    rounds the tracing of a face state differently can be held to the reference there (the contracted
    tile and wave kernels were 0.05 to 0.49 off on the MI355X at 29 x 61, 31 x 55, 35 x 113 and 70 x 58,
    and equal to it on the emulator, whose contracted build has no fma).  The state of the list does not
    move by more than 1e-12"""
    shape = (31, 55, 0)
    nx, ny, _ = shape
    for towards_wall in (True, False):
        case = ("super", cc.BCS[3], 2, 1, 0.0, "CGF", -1.e200)         # (y low: reflect)
        state = cc.make_state("super", nx, ny, *seams(shape))
        if towards_wall:
            state[..., 3] = -state[..., 3]                              # (sph_cases.make_state's own)
        U0 = oracle_fill(state, shape, case)
        assert (U0[I][:, 0, 3] < 0).all() == towards_wall
        dt = orc.comp_dt(U0, nx, ny, NG, *cc.spacing(nx, ny), cc.GAMMA, cc.CFL)
        Uo = U0.copy()
        assert orc.comp_step(Uo, oracle_params(shape, case), dt)[0] == 0 and np.isfinite(Uo).all()
        A = U0.copy()
        cell = (NG + nx // 3, NG - 1, 3)                                 # a ghost cell beside the wall
        A[cell] = np.nextafter(A[cell], 10.0)
        assert orc.comp_step(A, oracle_params(shape, case), dt)[0] == 0
        move = fast_err(A, Uo)
        print("supersonic gas", "into" if towards_wall else "away from", "the reflecting side: an ulp in a ghost cell "
              f"moves the oracle by {move:.3e}")
        assert (move > 1e-2) if towards_wall else (move < 1e-12), (towards_wall, move)


# ---------------------------------------------------------------- one step
def one_step_checks(dev, shape, case, report=None):
    """the fill, dt, the staged set, the tile kernel and k_ctu_wave (bit-faithful), both one-launch
    kernels contracted, against the oracle; the launch count; a second call from the same input"""
    exact = dev.kind == "emu"
    U0, Uo, dt, rc = oracle_case(shape, case)
    tag = (shape, case)
    s = device_state(dev, shape, case)

    def run(ks, fast, prof=False):
        P = device_params(shape, case, kernel_set=ks, fast_math=fast)
        s.upload(U0)
        s.fill_bc()
        if prof:
            rep = profiled_step(dev, s, P, dt)
            return s.download(), rep
        s.comp_step(P, dt)
        return s.download()

    s.upload(cc.make_state(case[0], shape[0], shape[1], *seams(shape)))
    s.fill_bc()
    assert np.array_equal(bits(s.download()), bits(U0)), (tag, "the device's fill is not the oracle's")
    dtd = s.comp_dt(device_params(shape, case, kernel_set=0), cc.CFL)
    assert dtd == dt if exact else abs(dtd / dt - 1) <= TOL_EXACT, (tag, dtd, dt)
    staged = run(0, 0)
    tile = run(1, 0)
    wave, rep = run(2, 0, prof=True)
    ftile = run(1, 1)
    fwave = run(2, 1)
    errs = [exact_err(U, Uo) for U in (staged, tile, wave)]
    ferrs = [fast_err(U, Uo) for U in (ftile, fwave)]
    print(f"{shape} {case}: dt {dtd!r} oracle {dt!r}; staged / tile / k_ctu_wave err {errs[0]:.3e} {errs[1]:.3e} "
          f"{errs[2]:.3e}, contracted tile / k_ctu_wave {ferrs[0]:.3e} {ferrs[1]:.3e}")
    if report is not None:
        report.append((shape, case, errs, ferrs))
    assert wave_alone(rep), (tag, rep)
    for what, U, err in zip(("staged", "tile", "k_ctu_wave"), (staged, tile, wave), errs):
        if exact:
            assert np.array_equal(U[I], Uo[I]), (tag, what, err, np.argwhere(U[I] != Uo[I])[:5])
        else:
            assert err <= TOL_EXACT, (tag, what, err)
    # the one-launch kernels against the staged set: the whole array, ghost frame included
    assert np.array_equal(tile, staged), (tag, np.argwhere(tile != staged)[:5])
    assert np.array_equal(wave, staged), (tag, np.argwhere(wave != staged)[:5])
    assert max(ferrs) <= TOL_FAST, (tag, ferrs)
    # the same step again from the same input: the same bits (priority board, LDS stash, reduction buffer reused)
    assert np.array_equal(bits(run(2, 0)), bits(wave)), tag
    assert np.array_equal(bits(run(2, 1)), bits(fwave)), tag


@pytest.mark.parametrize("name", shape_list(), ids=SHAPE_IDS)
def test_ctu_step_vs_oracle(dev, name):
    """one step of every case of a shape (every state; boundary mixes, solvers, limiter, flattening and
    gravity in turn): the device's fill against the oracle's, comp_dt against orc.comp_dt; the interior
    of the staged set, the tile kernel and k_ctu_wave against the oracle (equal on the emulator,
    <= TOL_EXACT on the GPU); both one-launch kernels equal to the staged set over the whole array;
    k_ctu_wave launched exactly once and nothing of the other sets; the contracted tile and wave
    kernels element-wise <= TOL_FAST with comp_floors; a second call giving the same bits"""
    shape = resolve(name)
    report = []
    for case in cc.cases_of(shape, shape_list().index(name)):
        one_step_checks(dev, shape, case, report)
    worst = max(report, key=lambda r: max(r[3]))
    print(f"largest contracted error of {shape}: {max(worst[3]):.3e} ({worst[1]})")


# ---------------------------------------------------------------- the slab launch order
@pytest.mark.parametrize("name", ["allcut", "mixed"])
def test_ctu_step_slab_launch_order(dev, name):
    """a state with neighbours set and no communicator (set_neighbours(0, 0): the launch order only)
    takes no cut strips and its boundary strips first: on the shape that has cut strips on THIS device
    the step gives the bits of the single-domain step, in both builds, by k_ctu_wave alone"""
    cus = dev.info()["compute_units"]
    shape = resolve(name, cus)
    nx, ny, mr = shape
    assert plan(nx, ny, cus, mr)["n_extra"] > 0 and plan(nx, ny, cus, mr, True)["n_extra"] == 0
    case = ("super", cc.BCS[1] if name == "mixed" else cc.BCS[2], 1, 1, cc.GRAV, "HLLC", -1.e200)
    dx, dy = cc.spacing(nx, ny)
    U0 = oracle_fill(cc.make_state("super", nx, ny, [nx // 2], [cc.WOUT]), shape, case)
    dt = orc.comp_dt(U0, nx, ny, NG, dx, dy, cc.GAMMA, cc.CFL)
    for fastm in (0, 1):
        P = device_params(shape, case, kernel_set=2, fast_math=fastm)
        out = []
        for slab in (False, True):
            s = device_state(dev, shape, case)
            if slab:
                s.set_neighbours(0, 0)
            s.upload(U0)
            s.fill_bc()
            rep = profiled_step(dev, s, P, dt)
            assert wave_alone(rep, slab), rep
            out.append(s.download())
        assert np.array_equal(bits(out[0]), bits(out[1])), (fastm, np.argwhere(out[0] != out[1])[:5])


# ---------------------------------------------------------------- the large shapes of 256 compute units
def oracle_window(U0, shape, case, dt, rows, cols):
    """the oracle's step of the cells rows x cols (offsets from ilo / jlo, half-open) as a grid of its own
    whose ghost cells are the cells around it in the filled array U0; a side of the window that is a side
    of the grid (and not periodic) keeps its boundary type, the others are outflow.  -> (result, mask of the cells that are
    the grid's own step: all but a margin of NG cells at the inner sides, where the source's ghost cells and
    the upper faces' viscosity are the window's)"""
    nx, ny, _ = shape
    kind, bcs, lim, flat, grav, solver, sd = case
    (r0, r1), (c0, c1) = rows, cols
    dx, dy = cc.spacing(nx, ny)
    sub = np.ascontiguousarray(U0[r0:r1 + 2 * NG, c0:c1 + 2 * NG])
    # (a periodic side is an inner one: the window does not hold the other end of the grid)
    inner = tuple(cutoff or b == "periodic" for cutoff, b in zip((r0 > 0, r1 < nx, c0 > 0, c1 < ny), bcs))
    wb = tuple("outflow" if cutoff else b for cutoff, b in zip(inner, bcs))
    P = orc.comp_params(r1 - r0, c1 - c0, NG, dx, dy, gamma=cc.GAMMA, limiter=lim, use_flattening=flat,
                        grav=grav, small_dens=sd, bcs=wb, riemann=solver)
    assert orc.comp_step(sub, P, dt)[0] == 0
    mask = np.ones((r1 - r0, c1 - c0), dtype=bool)
    if inner[0]: mask[:NG] = False
    if inner[1]: mask[-NG:] = False
    if inner[2]: mask[:, :NG] = False
    if inner[3]: mask[:, -NG:] = False
    return sub[I], mask


BIG = {"allcut": ("zeros", 2, 2, 1, cc.GRAV, "HLLC"), "mixed": ("super", 1, 0, 1, 0.0, "CGF"),
       "noprio": ("smooth", 3, 1, 0, cc.GRAV, "HLLC_lm"), "short": ("super", 1, 2, 1, cc.GRAV, "HLLC")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BIG))
def test_ctu_step_large_shape_256_cus(hip, name):
    """the searched shapes of the device's own compute units (256 on the MI355X: 0.2 to 6.7 million
    cells), each through its path (test_wave_plan_reaches_every_path): the bit-faithful k_ctu_wave
    against the tile kernel over the whole array, bit for bit -- the tile kernel is held to the oracle
    by everything above --, one launch; and the oracle on windows of rows and columns around the first
    seams of the path (the first short strip, the first cut, the second row strip) at the first, a
    middle and the last column strips: bit-faithful <= TOL_EXACT, contracted <= TOL_FAST"""
    cus = hip.info()["compute_units"]
    shape = resolve(name, cus)
    nx, ny, mr = shape
    g = plan(nx, ny, cus, mr)
    path = {"allcut": "all_cut", "mixed": "cut_and_regular", "noprio": "no_priority", "short": "short_tail"}[name]
    assert path in cc.paths_of(g, nx, mr), (shape, cus, g)
    kind, nbc, lim, flat, grav, solver = BIG[name]
    case = (kind, cc.BCS[nbc], lim, flat, grav, solver, -1.e200)
    regular, cut = cc.strips_of(g, nx)
    seam = regular[g["long_row_strips"]][0] if name == "short" else cut[1][0] if cut else regular[1][0]
    dx, dy = cc.spacing(nx, ny)
    state = cc.make_state(kind, nx, ny, [seam], [cc.WOUT]) if kind != "zeros" else \
        cc.make_state(kind, nx, ny, [seam, regular[1][0]], [cc.WOUT, ny - ny % cc.WOUT])
    U0 = oracle_fill(state, shape, case)
    dt = orc.comp_dt(U0, nx, ny, NG, dx, dy, cc.GAMMA, cc.CFL)
    s = device_state(hip, shape, case)
    out = {}
    for ks, fastm in ((1, 0), (2, 0), (2, 1)):
        s.upload(U0)
        s.fill_bc()
        rep = profiled_step(hip, s, device_params(shape, case, kernel_set=ks, fast_math=fastm), dt)
        assert ks != 2 or wave_alone(rep), rep
        out[ks, fastm] = s.download()
    assert np.array_equal(bits(out[1, 0]), bits(out[2, 0])), np.argwhere(out[1, 0] != out[2, 0])[:5]
    rows = (max(seam - 12, 0), min(seam + 12, nx))
    ncb = g["col_strips"]
    for cb in sorted({0, ncb // 2, ncb - 1}):
        cols = (max(cc.WOUT * cb - 12, 0), min(cc.WOUT * (cb + 1) + 12, ny))
        ref, mask = oracle_window(U0, shape, case, dt, rows, cols)
        W = (slice(NG + rows[0], NG + rows[1]), slice(NG + cols[0], NG + cols[1]))
        err = max(max_rel_err(out[2, 0][W][..., n][mask], ref[..., n][mask]) for n in range(4))
        fl = comp_floors(ref, cc.GAMMA)
        ferr = max(elementwise_err(out[2, 1][W][..., n][mask], ref[..., n][mask], fl[n]) for n in range(4))
        print(f"{shape} {case} ({path}) rows {rows} columns {cols}: k_ctu_wave err {err:.3e}, contracted {ferr:.3e}")
        assert mask.sum() >= 4 * cc.WOUT
        assert err <= TOL_EXACT, (cb, err)
        assert ferr <= TOL_FAST, (cb, ferr)


# ---------------------------------------------------------------- three steps, the device-side loop
# (the short-tail shape, a hundred thousand cells, stands where the rotation has no gravity: one run)
EVOLVE_SHAPES = [((31, 55, 0), "one_strip"), ((36, 60, 11), "joined_last"), (("short", 4), "short_tail"),
                 ((5, 57, 1), "one_row_strips"), ((12, 113, 3), "march_rows"), ((40, 169, 0), "regular_strips"),
                 (("allcut", 4), "all_cut"), (("mixed", 4), "cut_and_regular"), ((70, 57, 11), "last_ng"),
                 ((70, 58, 1), "no_priority")]
NSTEPS = 3


def evolve_checks(dev, shape, case, launches_of):
    """three steps of a case: the oracle loop, k_ctu_wave (bit-faithful) step by step against it, and
    comp_evolve with each step_launches of `launches_of` against the single steps; which launches a step
    of comp_evolve took is read from the profile"""
    nx, ny, mr = shape
    dx, dy = cc.spacing(nx, ny)
    Po = oracle_params(shape, case)
    U0 = cc.make_state(case[0], nx, ny, *seams(shape))
    Uo, pol_o, dto = U0.copy(), DtPolicy(1.e30, 0.1), []
    for _ in range(NSTEPS):
        oracle_fill(Uo, shape, case)
        dto.append(pol_o(orc.comp_dt(Uo, nx, ny, NG, dx, dy, cc.GAMMA, cc.CFL)))
        assert orc.comp_step(Uo, Po, dto[-1])[0] == 0
        pol_o.advance(dto[-1])
    assert np.isfinite(Uo).all()
    exact = dev.kind == "emu"
    P = device_params(shape, case, kernel_set=2, fast_math=0)
    s1 = device_state(dev, shape, case)
    s1.upload(U0)
    pol1, d1 = DtPolicy(1.e30, 0.1), []
    for _ in range(NSTEPS):
        s1.fill_bc()
        d1.append(pol1(s1.comp_dt(P, cc.CFL)))
        s1.comp_step(P, d1[-1])
        pol1.advance(d1[-1])
    U1 = s1.download()
    err = exact_err(U1, Uo)
    derr = float(np.abs(np.array(d1) / np.array(dto) - 1).max())
    print(f"{shape} {case}: three steps err {err:.3e}, dt err {derr:.3e}")
    if exact:
        assert d1 == dto, (d1, dto)
        assert np.array_equal(U1[I], Uo[I]), np.argwhere(U1[I] != Uo[I])[:5]
    else:
        assert derr <= TOL_EXACT, (d1, dto)
        assert err <= TOL_EXACT, err
    for launches in launches_of:
        s = device_state(dev, shape, case)
        s.upload(U0)
        pol = DtPolicy(1.e30, 0.1)
        dev.prof_enable(True)
        dev.prof_report()
        try:
            dts = list(s.comp_evolve(device_params(shape, case, kernel_set=2, fast_math=0, step_launches=launches),
                                     cc.CFL, pol, NSTEPS))
            rep = dev.prof_report()
        finally:
            dev.prof_enable(False)
        # one step kernel per step; a step of three launches has the fill-and-policy launch in front of it, a
        # step of one launch has none (the frame is filled once, behind the last step)
        assert rep.get("k_ctu_wave", (0, 0))[0] == NSTEPS and "k_ctu_fused" not in rep, (launches, rep)
        assert ("k_fill_frame2_policy" in rep) == (launches == 3), (launches, rep)
        assert dts == d1 and pol.t == pol1.t and pol.n == NSTEPS, (launches, dts, d1)
        U = s.download()
        assert np.array_equal(bits(U), bits(U1)), (launches, np.argwhere(U != U1)[:5])


@pytest.mark.parametrize("name,path", EVOLVE_SHAPES, ids=[p for _, p in EVOLVE_SHAPES])
def test_ctu_three_steps_and_evolve_vs_oracle(dev, name, path):
    """three steps with the driver's dt policy on the oracle and on the device, one shape of every
    path: k_ctu_wave (bit-faithful) step by step, and as comp_evolve(P, cfl, pol, 3) with step_launches
    3 (fill + frame, step, policy) and 1 (the step kernel alone: ghost cells through the boundary
    rules, the dt policy by its last wavefront, no short tail): dt lists and interiors equal to the
    oracle's on the emulator, within TOL_EXACT on the GPU; comp_evolve equal to the single steps over
    the whole array, ghost frame included, dt for dt.  A step with a source term reads ghost cells of its
    own and keeps its three launches whatever step_launches says (comp_api.hip: comp_can_fuse_fill): the
    cases of the rotation that carry gravity take step_launches 1 WITHOUT it, as a second run, and the
    profile says which launches a step took"""
    shape = resolve(name)
    nx, ny, mr = shape
    assert path in cc.paths_of(plan(nx, ny, 4, mr), nx, mr)
    n = [p for _, p in EVOLVE_SHAPES].index(path)
    lim, flat, grav = cc.PARAMS[n % len(cc.PARAMS)]
    kind = cc.STATES[n % len(cc.STATES)]
    case = (kind, cc.BCS[(n + 1) % len(cc.BCS)], lim, flat, grav, cc.SOLVERS[n % 3],
            cc.SMALL_DENS if kind == "floor" else -1.e200)
    if grav == 0.0:
        evolve_checks(dev, shape, case, (3, 1))
    else:
        evolve_checks(dev, shape, case, (3,))
        evolve_checks(dev, shape, case[:4] + (0.0,) + case[5:], (1,))
