"""The SphericalPolar step kernels -- the staged set, the one-launch tile kernel k_ctu_fused_sph and
the row-marching kernel k_sph_wave in its bit-faithful and contracted builds (csrc/comp_sph_wave.hip),
the device-side stepping loop on top of it -- against the C oracle orc.comp_step(..., geom=)
(oracle/pyro_oracle.c, pinned to the reference by tests/test_oracle_golden.py) at the seams of
k_sph_wave's launch geometry.

Shapes, states and parameters: tests/sph_cases.py.  Every path of the kernel's unit decoding is
reached for 4 compute units (the emulated device) and for 256 (the MI355X); the list is held to the
library's own geometry call (device.sph_wave_geometry: the code the step goes by), so a change of
wave_strip_rows or wave_fill_extra that drops a path fails without a launch.

The `dev` tests run on the emulated build here (bit for bit) and on the MI355X under -m gpu."""
import functools

import numpy as np
import pytest

import sph_cases as sc
from conftest import comp_floors, elementwise_err
from helpers import DtPolicy
from oracle import orc
from test_device_compressible import TOL_EXACT, TOL_FAST, comp_state

NG = sc.NG
I = (slice(NG, -NG), slice(NG, -NG))
SHAPE_IDS = [f"{a}x{b}m{m}" for a, b, m in sc.SHAPES] + ["mixed4"]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def geometry(nx, ny, cus, march_rows):
    from pyro2_amd import device
    return device.sph_wave_geometry(nx, ny, NG, cus, march_rows)


def resolve(shape, cus=4):
    if shape in ("mixed", "mixed4"):
        return sc.pick_mixed(geometry, cus)
    if shape == "noprio":
        return sc.pick_noprio(geometry, cus)
    return shape


def shape_list():
    return list(sc.SHAPES) + ["mixed4"]


def seams(shape):
    """row and column seams of a shape: of the strips of both devices"""
    nx, ny, mr = shape
    return sc.row_seams(nx, [geometry(nx, ny, cus, mr) for cus in (4, 256)]), sc.col_seams(ny)


@functools.lru_cache(maxsize=None)
def grid_geo(nx, ny):
    grid = sc.grid_of(nx, ny)
    geo = grid.device_geometry()
    assert "rowf" in geo and "colf" in geo
    return grid, geo, orc.Geom(geo, grid.xmin, grid.ymin)


def device_geo(nx, ny, fac):
    geo = grid_geo(nx, ny)[1]
    return geo if fac else {k: v for k, v in geo.items() if k not in ("rowf", "colf")}


def oracle_params(shape, case):
    nx, ny, _ = shape
    kind, bcs, lim, flat, grav, fac, sd = case
    grid = grid_geo(nx, ny)[0]
    return orc.comp_params(nx, ny, NG, grid.dx, grid.dy, gamma=sc.GAMMA, limiter=lim, use_flattening=flat,
                           grav=grav, small_dens=sd, bcs=tuple(bcs), riemann="CGF")


def oracle_fill(U, shape, case):
    nx, ny, _ = shape
    grid = grid_geo(nx, ny)[0]
    return orc.comp_fill_bc(U, nx, ny, NG, list(case[1]), sc.GAMMA, case[4], grid.dy, (0.0,) * 4)


@functools.lru_cache(maxsize=None)
def oracle_case(shape, case):
    """one oracle step of a case, computed once and shared (read-only): (filled input, result, dt, rc)"""
    nx, ny, _ = shape
    og = grid_geo(nx, ny)[2]
    rows, cols = seams(shape)
    U0 = oracle_fill(sc.make_state(case[0], nx, ny, rows, cols), shape, case)
    dt = orc.comp_dt_geom(U0, nx, ny, NG, og, sc.GAMMA, sc.CFL)
    Uo = U0.copy()
    rc, _ = orc.comp_step(Uo, oracle_params(shape, case), dt, geom=og)
    U0.flags.writeable = Uo.flags.writeable = False
    return U0, Uo, dt, rc


def device_params(shape, case, **kw):
    from pyro2_amd import device
    nx, ny, mr = shape
    kind, bcs, lim, flat, grav, fac, sd = case
    grid = grid_geo(nx, ny)[0]
    sol = sc.solid(bcs)
    if kw.get("kernel_set") == 2:
        kw.setdefault("march_rows", mr)
    return device.make_comp_params(grid.dx, grid.dy, gamma=sc.GAMMA, limiter=lim, use_flattening=flat, grav=grav,
                                   small_dens=sd, riemann="CGF", solid_xl=sol[0], solid_yl=sol[2], **kw)


def device_state(dev, shape, case):
    nx, ny, _ = shape
    grid = grid_geo(nx, ny)[0]
    s = comp_state(dev, nx, ny, list(case[1]))
    s.set_geometry(device_geo(nx, ny, case[5]), grid.xmin, grid.ymin)
    return s


def exact_err(U, Uo):
    """the measure of test_device_compressible.py's spherical tests: per variable, over the interior,
    against the variable's largest magnitude (at least 1e-3)"""
    scale = np.maximum(np.abs(Uo[I]).max(axis=(0, 1)), 1e-3)
    return float((np.abs(U - Uo)[I] / scale).max())


def fast_err(U, Uo):
    """element-wise with that file's floors (conftest.comp_floors: the ambient scales of the reference)"""
    fl = comp_floors(Uo[I], sc.GAMMA)
    return max(elementwise_err(U[I][..., n], Uo[I][..., n], fl[n]) for n in range(4))


# ---------------------------------------------------------------- the case list itself
def test_wave_geometry_reaches_every_path(dev):
    """no launch: the shapes of sph_cases.PATHS take the paths they are listed under, for 4 and for
    256 compute units, by the geometry the step itself goes by (pyrohip_sph_wave_geometry); the
    conditions of the two picked shapes hold; every shape of the list stands under a path; and the
    column and row counts sit around the strips they are for"""
    listed = set()
    for path, by_cus in sc.PATHS.items():
        for cus in (4, 256):
            assert by_cus[cus], (path, cus)
            for name in by_cus[cus]:
                shape = resolve(name, cus)
                nx, ny, mr = shape
                if cus == 4:
                    listed.add(shape)
                    assert shape in [resolve(s) for s in shape_list()], shape
                geo = geometry(nx, ny, cus, mr)
                regular, cut = sc.strips_of(geo, nx)
                assert path in sc.paths_of(geo, nx, mr), (path, shape, cus, geo)
                ncb, nsb, L = geo["col_strips"], geo["row_strips"], geo["rows_per_strip"]
                assert geo["slots"] == 8 * cus and ncb == -(-ny // sc.SWOUT)
                assert geo["wavefronts"] == ncb * nsb + geo["n_extra"]
                assert geo["prio_duty"] == (5 if geo["wavefronts"] <= 2 * geo["slots"] else 0)
                assert regular[0][0] == 0 and regular[-1][1] == nx
                assert all(a[1] == b[0] for a, b in zip(regular, regular[1:]))
                if path == "one_strip":
                    assert nx <= 32 and nsb == 1 and L == nx and geo["n_extra"] == 0
                if path == "joined_last":
                    tail = nx - nsb * L
                    assert 0 < tail < NG and regular[-1] == (nx - L - tail, nx), (shape, geo)
                if path == "last_ng":
                    assert nsb >= 2 and regular[-1] == (nx - NG, nx) and L > NG
                if path == "march_rows":
                    assert mr > 0 and L == mr and nsb >= 2 and geo["n_extra"] == 0
                if path == "one_row_strips":
                    # (a last strip of one row is shorter than the ghost width: it joins)
                    assert L == 1 and nsb == nx - 1 and regular[-1] == (nx - 2, nx)
                if path == "all_cut":
                    assert mr == 0 and geo["n_extra"] == ncb and nsb >= 2 and len(cut) == nsb + 1
                    assert min(b - a for a, b in cut) >= 8 and cut[0][0] == 0 and cut[-1][1] == nx
                if path == "cut_and_regular":
                    assert mr == 0 and 2 <= geo["n_extra"] <= ncb - 2 and nsb >= 2
                    assert geo["wavefronts"] == geo["slots"]
                    assert ny % sc.SWOUT not in (0,)              # with a ragged last column strip
                if path == "no_priority":
                    assert geo["wavefronts"] > 2 * geo["slots"] and geo["prio_duty"] == 0
    assert listed == {resolve(s) for s in shape_list()}, "a shape that stands under no path"
    # the two picked shapes: small on the emulated device, a few hundred thousand and a few million cells on 256
    assert np.prod(resolve("mixed", 4)[:2]) < 3e4
    assert np.prod(resolve("mixed", 256)[:2]) < 3e6 and np.prod(resolve("noprio", 256)[:2]) < 5e5
    assert all(nx * ny <= 1e4 for nx, ny, _ in sc.SHAPES)
    assert {ny for _, ny, _ in sc.SHAPES} >= {4, 55, 56, 57, 60, 64, 112, 113, 120, 169}
    assert {nx for nx, _, _ in sc.SHAPES} >= {4, 5, 8, 12, 31, 32, 33, 35, 36, 40, 66, 70}
    assert {mr for _, _, mr in sc.SHAPES} == {0, 1, 3, 5, 11}
    # every shape with two row strips or more and no march_rows takes the all-cut path on 256 compute units
    for nx, ny, mr in sc.SHAPES:
        g = geometry(nx, ny, 256, mr)
        if mr == 0 and g["row_strips"] >= 2:
            assert g["n_extra"] == g["col_strips"]


def test_oracle_floor_beside_odd_wall_turns_on_an_ulp(dev):
    """why no `floor` case has a floored cell in the row beside the oddly reflecting boundary, in the
    oracle alone: with such a cell (`floor_wall`: (ilo, jlo + 2)) the density of the face state at
    the boundary is negative, the two-shock solver's sound speed there is its floor 1e-10 and its
    star density is (pstar - p) 1e20 with pstar - p a cancellation residue.  One to eight ulps more
    energy in that cell move the oracle's own result between a few discrete answers that lie more
    than 1e-3 apart in the contracted build's measure (1.1e-2 with limiter 0 at 36 x 57, 1.2e-3 with
    limiter 2 at 5 x 57), seven decades above its bar: no build with another rounding can be held
    to the reference there.  The `floor` state itself moves by less than 1e-12"""
    for shape, lim in (((36, 57, 0), 0), ((5, 57, 1), 2)):
        og = grid_geo(*shape[:2])[2]
        for kind, sensitive in (("floor_wall", True), ("floor", False)):
            case = (kind, sc.BCS[0], lim, 1, 0.0, 1, sc.SMALL_DENS)
            U0, Uo, dt, rc = oracle_case(shape, case)
            assert rc == 0 and np.isfinite(Uo).all()
            cell = (NG, NG + 2, 1) if sensitive else (NG + 1, NG, 1)       # the energy of a floored cell
            assert U0[cell[:2]][0] < sc.SMALL_DENS
            A0, errs = np.array(U0), []
            for _ in range(8):
                A0[cell] = np.nextafter(A0[cell], 10.0)
                A = oracle_fill(A0.copy(), shape, case)
                assert orc.comp_step(A, oracle_params(shape, case), dt, geom=og)[0] == 0
                errs.append(fast_err(A, np.array(Uo)))
            print(shape, kind, "1 .. 8 ulps move the oracle by", ["%.1e" % e for e in errs])
            assert (max(errs) > 1e-3) if sensitive else (max(errs) < 1e-12), (shape, kind, errs)


def all_cases():
    return [(s, c) for n, s in enumerate(shape_list()) for c in sc.cases_of(resolve(s), n)]


def test_case_list_conditions(dev):
    """the oracle alone, over the whole list, no case left out: rc == 0, every result is finite,
    every step moves the interior by more than 1e-3 of its scale, the `floor` cases have interior
    densities below small_dens and the floor changes their result; and the list covers every
    state with every boundary mix, every limiter, flattening on and off, both values of grav, the
    geometry with and without its 1-d factors, on single and on several column strips"""
    seen = set()
    for name, case in all_cases():
        shape = resolve(name)
        kind, bcs, lim, flat, grav, fac, sd = case
        U0, Uo, dt, rc = oracle_case(shape, case)
        tag = (shape, case)
        assert rc == 0 and dt > 0, tag
        assert np.isfinite(Uo).all(), tag
        assert Uo[I][..., 0].min() > 0, tag
        scale = np.abs(U0[I]).max(axis=(0, 1))
        moved = (np.abs(Uo[I] - U0[I]).max(axis=(0, 1)) / np.maximum(scale, 1e-300))
        assert moved[:2].min() > 1e-3 and moved.max() > 1e-3, (tag, moved)
        if kind == "floor":
            assert sd == sc.SMALL_DENS and (U0[I][..., 0] < sd).sum() >= 2, tag
            assert U0[I][0, :, 0].min() > sd and U0[I][-1, :, 0].min() > sd, tag      # (see make_state)
            free = U0.copy()
            unfloored = list(case)
            unfloored[6] = -1.e200
            assert orc.comp_step(free, oracle_params(shape, tuple(unfloored)), dt, geom=grid_geo(*shape[:2])[2])[0] == 0
            assert not np.array_equal(free[I], Uo[I]), tag
        else:
            assert U0[I][..., 0].min() > sc.SMALL_DENS
        if kind == "zeros":
            for var in (2, 3):
                z = U0[I][..., var] == 0.0
                assert z.any() and np.signbit(U0[I][..., var][z]).any() and not np.signbit(U0[I][..., var][z]).all(), tag
        multi = shape[1] > sc.SWOUT
        seen |= {("state-bc", kind, bcs), ("lim", lim), ("flat", flat), ("grav", grav), ("fac", fac),
                 ("std-fac", lim == 2 and flat == 1, fac), ("state-cols", kind, multi), ("state-fac", kind, fac)}
    for kind in sc.STATES:
        assert all(("state-bc", kind, b) in seen for b in sc.BCS), kind
        assert all(("state-cols", kind, m) in seen for m in (False, True)), kind
        assert all(("state-fac", kind, f) in seen for f in (0, 1)), kind
    assert all(("lim", n) in seen for n in (0, 1, 2)) and all(("flat", n) in seen for n in (0, 1))
    assert ("grav", 0.0) in seen and ("grav", sc.GRAV) in seen
    assert all(("std-fac", a, b) in seen for a in (False, True) for b in (0, 1))


# ---------------------------------------------------------------- one step
def one_step_checks(dev, shape, case, report=None):
    """dt, the staged set, the tile kernel and k_sph_wave (bit-faithful and contracted) of one case
    against the oracle; the launch count; a second call from the same input"""
    exact = dev.kind == "emu"
    U0, Uo, dt, rc = oracle_case(shape, case)
    tag = (shape, case)
    s = device_state(dev, shape, case)

    def run(ks, fast, prof=False):
        P = device_params(shape, case, kernel_set=ks, fast_math=fast)
        s.upload(U0)
        s.fill_bc()
        if prof:
            dev.prof_enable(True)
            dev.prof_report()
        try:
            s.comp_step(P, dt)
            rep = dev.prof_report() if prof else None
        finally:
            if prof:
                dev.prof_enable(False)
        return (s.download(), rep) if prof else s.download()

    s.upload(U0)
    s.fill_bc()
    assert np.array_equal(bits(s.download()), bits(U0)), (tag, "the device's fill is not the oracle's")
    dtd = s.comp_dt(device_params(shape, case, kernel_set=0), sc.CFL)
    print(f"{shape} {case}: dt {dtd!r} oracle {dt!r}")
    assert dtd == dt if exact else abs(dtd / dt - 1) <= TOL_EXACT, (tag, dtd, dt)
    staged = run(0, 0)
    tile = run(1, 0)
    wave, rep = run(2, 0, prof=True)
    fast = run(2, 1)
    errs = [exact_err(U, Uo) for U in (staged, tile, wave)]
    ferr = fast_err(fast, Uo)
    print(f"{shape} {case}: staged / tile / k_sph_wave err {errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e}, "
          f"contracted k_sph_wave {ferr:.3e}")
    if report is not None:
        report.append((shape, case, errs, ferr))
    # the launch: k_sph_wave once and nothing of the other sets (the profile report has no grid size:
    # the unit count is held to the geometry call by the interiors above -- a unit left out is a strip not updated)
    assert rep.get("k_sph_wave", (0, 0))[0] == 1 and "k_sph_states" not in rep and "k_ctu_fused_sph" not in rep, (tag, rep)
    for what, U, err in zip(("staged", "tile", "k_sph_wave"), (staged, tile, wave), errs):
        if exact:
            assert np.array_equal(U[I], Uo[I]), (tag, what, err, np.argwhere(U[I] != Uo[I])[:5])
        else:
            assert err <= TOL_EXACT, (tag, what, err)
    # the one-launch kernels against the staged set: the whole array, ghost frame included
    assert np.array_equal(tile, staged), (tag, np.argwhere(tile != staged)[:5])
    assert np.array_equal(wave, staged), (tag, np.argwhere(wave != staged)[:5])
    assert ferr <= TOL_FAST, (tag, ferr)
    # the same step again from the same input: the same bits (priority board, LDS stash, reduction buffer reused)
    assert np.array_equal(bits(run(2, 0)), bits(wave)), tag
    assert np.array_equal(bits(run(2, 1)), bits(fast)), tag


@pytest.mark.parametrize("name", shape_list(), ids=SHAPE_IDS)
def test_sph_step_vs_oracle(dev, name):
    """one step of every case of a shape (every state; boundary mixes, limiter, flattening, gravity and
    the geometry's form in turn): comp_dt against orc.comp_dt_geom; the interior of the staged set,
    the tile kernel and k_sph_wave against the oracle (equal on the emulator, <= TOL_EXACT in the
    measure of the spherical tests of test_device_compressible.py on the GPU); both one-launch
    kernels equal to the staged set over the whole array; k_sph_wave launched exactly once; the
    contracted k_sph_wave element-wise <= 1e-10 with comp_floors; a second call giving the same bits.
    (The `sedov` cases with limiter 0 and reflect-odd at 8 x 169 and 12 x 113 found hydro.h: pvel's zero
    sign in ghost cells of negative density on the MI355X: 5e-8 and 2.5e-7 in all three kernel sets.)"""
    shape = resolve(name)
    report = []
    for case in sc.cases_of(shape, shape_list().index(name)):
        one_step_checks(dev, shape, case, report)
    worst = max(report, key=lambda r: r[3])
    print(f"largest contracted error of {shape}: {worst[3]:.3e} ({worst[1]})")


def big_shape_check(hip, shape, case, path):
    """a large shape on the MI355X: k_sph_wave once in each build, and the oracle once"""
    nx, ny, mr = shape
    cus = hip.info()["compute_units"]
    geo = geometry(nx, ny, cus, mr)
    assert path in sc.paths_of(geo, nx, mr), (shape, cus, geo)
    U0, Uo, dt, rc = oracle_case(shape, case)
    assert rc == 0 and np.isfinite(Uo).all()
    s = device_state(hip, shape, case)
    out = []
    for fastm in (0, 1):
        s.upload(U0)
        s.fill_bc()
        hip.prof_enable(True)
        hip.prof_report()
        try:
            s.comp_step(device_params(shape, case, kernel_set=2, fast_math=fastm), dt)
            rep = hip.prof_report()
        finally:
            hip.prof_enable(False)
        assert rep.get("k_sph_wave", (0, 0))[0] == 1, rep
        out.append(s.download())
    err, ferr = exact_err(out[0], Uo), fast_err(out[1], Uo)
    print(f"{shape} {case} ({path}, {geo}): k_sph_wave err {err:.3e}, contracted {ferr:.3e}")
    assert err <= TOL_EXACT, err
    assert ferr <= TOL_FAST, ferr


@pytest.mark.gpu
def test_sph_step_cut_and_regular_256_cus(hip):
    """cut and regular column strips in one launch on 256 compute units: 36 rows, some 38000
    columns (test_wave_geometry_reaches_every_path), the `zeros` state between reflecting walls"""
    shape = resolve("mixed", 256)
    big_shape_check(hip, shape, ("zeros", sc.BCS[2], 2, 1, sc.GRAV, 1, -1.e200), "cut_and_regular")


@pytest.mark.gpu
def test_sph_step_no_priority_256_cus(hip):
    """more wavefronts than two rounds of slots on 256 compute units (1-row strips): no priority
    board is taken; the `super` state, periodic in theta"""
    shape = resolve("noprio", 256)
    big_shape_check(hip, shape, ("super", sc.BCS[1], 1, 0, 0.0, 1, -1.e200), "no_priority")


# ---------------------------------------------------------------- the CFL minimum the step leaves
CFL_SHAPES = [(8, 169, 0), (36, 57, 0), (35, 60, 11), (12, 113, 3)]


@pytest.mark.parametrize("bcs", sc.BCS, ids=["-".join(b) for b in sc.BCS])
@pytest.mark.parametrize("shape", CFL_SHAPES, ids=[f"{a}x{b}m{m}" for a, b, m in CFL_SHAPES])
def test_sph_cached_dt_vs_oracle(dev, shape, bcs):
    """after a fuse_fill step of k_sph_wave the cached comp_dt (the kernel's CFL minimum, the ghost
    cells of the new state with their own Lx, Ly included: sphf_ghost_cfl) against the oracle's
    comp_dt_geom of the new state after the oracle's fill: bit for bit in the bit-faithful build,
    1e-13 relative in the contracted one; `smooth` and `super` states at multi-strip shapes"""
    assert shape in sc.SHAPES
    nx, ny, mr = shape
    og = grid_geo(nx, ny)[2]
    for n, kind in enumerate(("smooth", "super")):
        lim, flat, grav, fac = sc.PARAMS[(sc.SHAPES.index(shape) + 2 * n) % len(sc.PARAMS)]
        case = (kind, bcs, lim, flat, grav, fac, -1.e200)
        U0, Uo, dt, rc = oracle_case(shape, case)
        assert rc == 0
        for fastm in (0, 1):
            s = device_state(dev, shape, case)
            s.upload(U0)
            s.fill_bc()
            P = device_params(shape, case, kernel_set=2, fast_math=fastm, fuse_fill=1)
            s.comp_step(P, dt)
            assert s.comp_dt_is_cached()
            cached = s.comp_dt(P, sc.CFL)
            U = oracle_fill(s.download(), shape, case)
            fresh = orc.comp_dt_geom(U, nx, ny, NG, og, sc.GAMMA, sc.CFL)
            print(f"{shape} {case} fast_math {fastm}: cached {cached!r}, oracle {fresh!r}")
            if fastm:
                assert abs(cached / fresh - 1) <= 1e-13, (case, cached, fresh)
            else:
                assert cached == fresh, (case, cached, fresh)


# ---------------------------------------------------------------- three steps, the device-side loop
EVOLVE_SHAPES = [((31, 55, 0), "one_strip"), ((35, 60, 11), "joined_last"), ((40, 113, 0), "all_cut"),
                 ("mixed4", "cut_and_regular")]
NSTEPS = 3


@pytest.mark.parametrize("name,path", EVOLVE_SHAPES, ids=[p for _, p in EVOLVE_SHAPES])
def test_sph_three_steps_and_evolve_vs_oracle(dev, name, path):
    """three steps with the driver's dt policy on the oracle and on the device, by k_sph_wave step by
    step and as comp_evolve(P, cfl, pol, 3): bit-faithful build: dt lists and interiors equal on the
    emulator, within TOL_EXACT on the GPU; comp_evolve equal to the single steps over the whole
    array in both builds"""
    shape = resolve(name)
    nx, ny, mr = shape
    assert path in sc.paths_of(geometry(nx, ny, 4, mr), nx, mr)
    n_shape = [p for _, p in EVOLVE_SHAPES].index(path)
    lim, flat, grav, fac = sc.PARAMS[n_shape]
    case = (("smooth", "zeros", "floor", "super")[n_shape], sc.BCS[n_shape % 3], lim, flat, grav, fac,
            sc.SMALL_DENS if n_shape == 2 else -1.e200)
    og = grid_geo(nx, ny)[2]
    Po = oracle_params(shape, case)
    rows, cols = seams(shape)
    U0 = sc.make_state(case[0], nx, ny, rows, cols)
    Uo, pol_o, dto = U0.copy(), DtPolicy(1.e30, 0.1), []
    for _ in range(NSTEPS):
        oracle_fill(Uo, shape, case)
        dto.append(pol_o(orc.comp_dt_geom(Uo, nx, ny, NG, og, sc.GAMMA, sc.CFL)))
        assert orc.comp_step(Uo, Po, dto[-1], geom=og)[0] == 0
        pol_o.advance(dto[-1])
    assert np.isfinite(Uo).all()
    exact = dev.kind == "emu"
    for fastm in (0, 1):
        P = device_params(shape, case, kernel_set=2, fast_math=fastm)
        s1 = device_state(dev, shape, case)
        s1.upload(U0)
        pol1, d1 = DtPolicy(1.e30, 0.1), []
        for _ in range(NSTEPS):
            s1.fill_bc()
            d1.append(pol1(s1.comp_dt(P, sc.CFL)))
            s1.comp_step(P, d1[-1])
            pol1.advance(d1[-1])
        U1 = s1.download()
        s = device_state(dev, shape, case)
        s.upload(U0)
        pol = DtPolicy(1.e30, 0.1)
        dts = list(s.comp_evolve(P, sc.CFL, pol, NSTEPS))
        assert dts == d1 and pol.t == pol1.t and pol.n == NSTEPS, (fastm, dts, d1)
        assert np.array_equal(bits(s.download()), bits(U1)), fastm
        if fastm:
            continue
        err = exact_err(U1, Uo)
        derr = float(np.abs(np.array(d1) / np.array(dto) - 1).max())
        print(f"{shape} {case}: three steps err {err:.3e}, dt err {derr:.3e}")
        if exact:
            assert d1 == dto, (d1, dto)
            assert np.array_equal(U1[I], Uo[I]), np.argwhere(U1[I] != Uo[I])[:5]
        else:
            assert derr <= TOL_EXACT, (d1, dto)
            assert err <= TOL_EXACT, err


# ---------------------------------------------------------------- an invalid state in every kind of unit
def invalid_placements():
    """(what, shape, (row, column) as offsets from (ilo, jlo))"""
    return [("second column strip", (8, 169, 0), (3, sc.SWOUT + 2)),
            ("last column of a ragged last column strip", (70, 57, 11), (40, 56)),
            ("extra row strip of a cut column strip", (36, 57, 0), (30, 20)),
            ("joined tail of the last row strip", (35, 60, 11), (34, 58))]


@pytest.mark.parametrize("fastm", [0, 1])
@pytest.mark.parametrize("n", range(4), ids=["col_strip_2", "ragged_last_col", "extra_row_strip", "joined_tail"])
def test_sph_invalid_state_in_every_unit_kind(dev, n, fastm):
    """one interior cell of negative density where the named kind of unit of k_sph_wave reads it as
    its own: ERR_STATE from kernel_set 2, the state unchanged (as test_spherical_invalid_cases on
    its single-strip grid), and a non-zero return of the oracle for the same input"""
    from pyro2_amd._lib import ERR_STATE, PyroHipError
    what, shape, (i, j) = invalid_placements()[n]
    nx, ny, mr = shape
    cus = dev.info()["compute_units"]
    geo = geometry(nx, ny, cus, mr)
    regular, cut = sc.strips_of(geo, nx)
    # the cell lies where the name says, on this device
    if n == 0:
        assert geo["col_strips"] >= 2 and sc.SWOUT <= j < 2 * sc.SWOUT
    elif n == 1:
        assert j == ny - 1 and ny % sc.SWOUT == 1
    elif n == 2:
        assert geo["n_extra"] == geo["col_strips"] and cut[-1][0] <= i < cut[-1][1] and j < sc.SWOUT
    else:
        assert geo["n_extra"] == 0 and regular[-1][0] + geo["rows_per_strip"] <= i < nx
    case = ("smooth", sc.BCS[n % 3], 2, 1, 0.0, n % 2, -1.e200)
    U0 = np.array(oracle_case(shape, case)[0])
    U0[NG + i, NG + j, 0] = -0.5
    oracle_fill(U0, shape, case)
    dt = 0.5 * oracle_case(shape, case)[2]
    assert orc.comp_step(U0.copy(), oracle_params(shape, case), dt, geom=grid_geo(nx, ny)[2])[0] != 0
    s = device_state(dev, shape, case)
    s.upload(U0)
    s.fill_bc()
    pre = s.download()
    assert np.array_equal(bits(pre), bits(U0))
    with pytest.raises(PyroHipError) as ei:
        s.comp_step(device_params(shape, case, kernel_set=2, fast_math=fastm), dt)
    assert ei.value.code == ERR_STATE, what
    assert np.array_equal(bits(s.download()), bits(pre)), what
    assert not s.comp_dt_is_cached(), what
