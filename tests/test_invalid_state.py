"""The invalid-state contract of the compressible kernels.

The reference refuses to step a state whose interior has min(rho) <= 0 or
min(e) <= 0 (compressible/simulation.py:68-71; numpy minima, so a NaN fails
too).  Every step path here answers such a state with PYROHIP_ERR_STATE and
leaves the state of before the failing step behind.

What a case's verdict IS comes from the reference, recorded by
oracle/gen_invalid_golden.py in tests/golden/comp_invalid_cases.npz (cases:
tests/invalid_cases.py).  The CPU pins hold a numpy restatement and the C
oracle to those verdicts; the device matrix holds every kernel path, both
builds, to them -- one bad cell at the middle, the corners and edges of the
grid and on either side of every strip and tile seam of the kernels.

The fast build's arithmetic (and its -fno-honor-nans unit) exists on the GPU
only: the emulator runs the fast_math = 1 code paths with true divisions, the
`hip` legs are what tests the fast build's NaN handling.

A test loops over its cases and reports every failing one, so that a run on a
broken library names the whole hole.
"""
import numpy as np
import pytest

import invalid_cases as ic
from conftest import max_rel_err
from helpers import RK_TABLEAU, DtPolicy, meta_to_params
from oracle import orc
from pyro2_amd import device
from pyro2_amd._lib import ERR_STATE, PyroHipError
from test_device_compressible import (TOL_EXACT, TOL_FAST, SPH_NAMES, assert_state_close, comp_state,
                                      dev_params, kset_kw)

NG = ic.NG
INT = (slice(NG, -NG), slice(NG, -NG))
BCS = ["outflow"] * 4


def same_bits(a, b):
    """bit-identical, NaN payloads and the sign of zero included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def ndiff(a, b):
    return int((np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)).sum())


def report(fails):
    """the failures of a loop over cases, as text: how many of which sort, and every one of them"""
    from collections import Counter
    sorts = Counter(" ".join(str(x) for x in f[4:] if isinstance(x, str)) for f in fails)
    return "\n".join([f"{len(fails)} failures"] + [f"  {n:4d} x {k}" for k, n in sorts.items()] +
                     ["  " + repr(f) for f in fails])


def outflow_fill(U, ng=NG):
    """fill_BC of four outflow sides, x first (mesh/patch.py fill_BC)"""
    U = U.copy()
    U[:ng] = U[ng]
    U[-ng:] = U[-ng - 1]
    U[:, :ng] = U[:, ng:ng + 1]
    U[:, -ng:] = U[:, -ng - 1:-ng]
    return U


def cart_meta():
    return np.array([ic.NX, ic.NY, NG, 1.0 / ic.NX, 1.0 / ic.NY, ic.GAMMA, 2, 1, 0.75, 0.85, 0.33, 0.1, 0.0, 0.8])


def fixture_cases(g, sph=False):
    """[(kind, i, j, [verdict per small_dens])] of the fixture, checked against the table"""
    pre = "sph_" if sph else ""
    kinds = [str(k) for k in g["kinds"]]
    assert tuple(kinds) == ic.KINDS
    assert tuple(g["small_dens"]) == ic.SMALL_DENS and int(g["seed"]) == ic.SEED
    table = ic.case_table(ic.sph_positions(*[int(n) for n in g["sph_grid"]])) if sph else ic.case_table()
    rows = [(kinds[k], int(i), int(j)) for k, i, j in g[pre + "cases"]]
    assert rows == [tuple(c) for c in table], "the fixture is not the one of this case table: regenerate it"
    return [(k, i, j, [int(v) for v in vs]) for (k, i, j), vs in zip(rows, g[pre + "verdict"])]


def device_cases(g, sph=False):
    """(kind, i, j, small_dens, verdict): every case under the default floor, every kind at the
    first position under small_dens = 1e-4 as well (the floor acts on one cell's density: what it
    does there does not depend on where the cell is)"""
    out = []
    for n, (k, i, j, vs) in enumerate(fixture_cases(g, sph)):
        out.append((k, i, j, ic.SMALL_DENS[0], vs[0]))
        if n < len(ic.KINDS):
            out.append((k, i, j, ic.SMALL_DENS[1], vs[1]))
    return out


# ---------------------------------------------------------------------------
# CPU pins
# ---------------------------------------------------------------------------
def test_case_table_covers_the_seams():
    """the positions hold both sides of every seam the kernels have on this grid"""
    pos = set(ic.positions())
    im, jm = ic.NX // 2, ic.NY // 2
    wg = {mr: device_geometry_rows(mr) for mr in (0, 11)}
    for mr, (L, nsb, ncb) in wg.items():
        assert ncb == 3 and ic.NY % ic.COL_STRIP != 0            # three column strips, a ragged one
        assert nsb >= 3 and (ic.NX - (nsb - 1) * L) != L         # a last strip of its own length
        for k in range(1, nsb):
            assert {(k * L - 1, jm), (k * L, jm)} <= pos, (mr, k)
    for j in (56, 112, 30, 60, 90, 120):
        assert {(im, j - 1), (im, j)} <= pos
    for i in (14, 28, 42):
        assert {(i - 1, jm), (i, jm)} <= pos
    assert {(0, 0), (0, ic.NY - 1), (ic.NX - 1, 0), (ic.NX - 1, ic.NY - 1)} <= pos


def device_geometry_rows(march_rows):
    """(rows per strip, row strips, column strips) of the row-marching kernel, from the library"""
    import os
    import sys
    from pyro2_amd import _lib
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    import build_emu
    if _lib._lib is None:
        _lib.use_library(build_emu.build(), allow_backends=("host-emu",))
    w = device.comp_wave_geometry(ic.NX, ic.NY, NG, 0, march_rows)
    return w["rows_per_strip"], w["row_strips"], w["col_strips"]


def test_numpy_restatement_agrees_with_the_reference(golden):
    """np.maximum for the floor, the where= divisions, the .min() of the interior: the verdict
    of every recorded case, both floors, both grids"""
    g = golden("comp_invalid_cases")
    base = ic.base_state()
    n = {0: 0, 1: 0}
    for k, i, j, vs in fixture_cases(g):
        U = ic.apply_case(base, k, i, j)
        for sd, v in zip(ic.SMALL_DENS, vs):
            assert ic.numpy_verdict(U, sd) == v, (k, i, j, sd)
            n[v] += 1
    assert n[0] >= 4 and n[1] >= 150          # both sides of the edge are in the table
    sb = sph_base(golden)[0]
    for k, i, j, vs in fixture_cases(g, sph=True):
        U = ic.apply_case(sb, k, i, j)
        for sd, v in zip(ic.SMALL_DENS, vs):
            assert ic.numpy_verdict(U, sd) == v, ("sph", k, i, j, sd)
    # the two valid neighbours of the edge are accepted, everything else is not
    for k, i, j, vs in fixture_cases(g):
        assert vs == ([0, 0] if k.startswith("ok_") else [1, 1]), (k, vs)


def test_oracle_agrees_with_the_reference(golden):
    """orc.comp_step and orc.comp_rk_rhs return rc = the reference's verdict for every case
    (the floor of clean_state is np.maximum: it keeps a NaN)"""
    g = golden("comp_invalid_cases")
    base = ic.base_state()
    meta = cart_meta()
    fails = []
    for k, i, j, vs in fixture_cases(g):
        U = ic.apply_case(base, k, i, j)
        for sd, v in zip(ic.SMALL_DENS, vs):
            P, cfl = meta_to_params(meta, BCS, small_dens=sd)
            rc, _ = orc.comp_step(U.copy(), P, 1.e-4)
            rk, _ = orc.comp_rk_rhs(U.copy(), P)
            if (rc, rk) != (v, v):
                fails.append((k, i, j, sd, "reference", v, "comp_step", rc, "comp_rk_rhs", rk))
    assert not fails, report(fails)


def test_spherical_oracle_agrees_with_the_reference(golden):
    g = golden("comp_invalid_cases")
    sb, meta, bcs, geom, _ = sph_base(golden)
    fails = []
    for k, i, j, vs in fixture_cases(g, sph=True):
        U = ic.apply_case(sb, k, i, j)
        for sd, v in zip(ic.SMALL_DENS, vs):
            P, cfl = meta_to_params(meta, bcs, riemann="CGF", small_dens=sd)
            rc, _ = orc.comp_step(U.copy(), P, 1.e-5, geom=geom)
            if rc != v:
                fails.append((k, i, j, sd, "reference", v, "oracle", rc))
    assert not fails, report(fails)


def sph_base(golden):
    """the SphericalPolar base state: the initial condition of the reference's spherical sedov
    set-up (golden file comp_spherical, case 0 -- what the generator perturbed), ghost cells filled"""
    from test_oracle_golden import sph_geom
    gs = golden("comp_spherical")
    pre = "c0_"
    meta = gs[pre + "meta"]
    bcs = [str(b) for b in gs[pre + "bc"]]
    assert (int(meta[0]), int(meta[1])) == tuple(int(n) for n in golden("comp_invalid_cases")["sph_grid"])
    U = np.nan_to_num(np.ascontiguousarray(gs[pre + "ic"], dtype=np.float64))
    orc.comp_fill_bc(U, int(meta[0]), int(meta[1]), NG, bcs, meta[5], meta[12], meta[4])
    return U, meta, bcs, sph_geom(gs, pre), gs


# ---------------------------------------------------------------------------
# the device matrix
# ---------------------------------------------------------------------------
def expect_rejected_step(tag, s, U, step, cached, fails):
    """upload, fill, step: ERR_STATE, the state (ghost cells too) bit for bit what it was, and
    no CFL minimum kept for the next dt"""
    s.upload(U)
    s.fill_bc()
    pre = s.download()
    if not same_bits(pre[INT], U[INT]):
        fails.append(tag + ("the fill changed the interior",))
    try:
        step()
        fails.append(tag + ("no error",))
        return
    except PyroHipError as e:
        if e.code != ERR_STATE:
            raise
    post = s.download()
    if not same_bits(post, pre):
        fails.append(tag + ("state changed", ndiff(post[INT], pre[INT]), "interior cells",
                            ndiff(post, pre) - ndiff(post[INT], pre[INT]), "ghost cells"))
    if cached():
        fails.append(tag + ("a CFL minimum is cached after the error",))


def expect_rejected_evolve(tag, s, s2, U, evolve, fails, max_steps=4, again=True):
    """the same state handed to a device-side run: ERR_STATE, no step done, clock untouched, the
    state is the upload with its ghost cells filled; and again on the same object (`again`: the
    cases of the first position do that, to keep the emulator's time down)"""
    s2.upload(U)
    s2.fill_bc()
    want = s2.download()
    s.upload(U)
    for attempt in ((1, 2) if again else (1,)):
        pol = DtPolicy(1.e30)
        pol.t, pol.n, pol.dt_old = 0.25, 3, 1.e-3
        try:
            evolve(pol, max_steps)
            fails.append(tag + ("evolve", attempt, "no error", pol.n))
            return
        except PyroHipError as e:
            if e.code != ERR_STATE:
                raise
            if e.steps_done != 0 or len(e.dts) != 0:
                fails.append(tag + ("evolve", attempt, "steps_done", e.steps_done))
        if (pol.n, pol.t) != (3, 0.25):
            fails.append(tag + ("evolve", attempt, "the clock moved", pol.n, pol.t))
        got = s.download()
        if not same_bits(got, want):
            fails.append(tag + ("evolve", attempt, "state changed", ndiff(got[INT], want[INT]), "interior cells",
                                ndiff(got, want) - ndiff(got[INT], want[INT]), "ghost cells"))
        if s.comp_dt_is_cached():
            fails.append(tag + ("evolve", attempt, "a CFL minimum is cached after the error",))


def check_accepted(tag, dev, U1, Uo, fast, fails):
    """exact build: the oracle's step, bit for bit on the emulator and within TOL_EXACT on the
    GPU; fast build: a finite result (its 1e-10 bar is not defined this close to the edge)"""
    if fast:
        if not np.isfinite(U1[INT]).all():
            fails.append(tag + ("not finite",))
        return
    if dev.kind == "emu":
        if not np.array_equal(U1[INT], Uo[INT]):
            fails.append(tag + ("not the oracle's step", ndiff(U1[INT], Uo[INT])))
    else:
        err = max(max_rel_err(U1[INT][..., n], Uo[INT][..., n]) for n in range(4))
        if not err <= TOL_EXACT:
            fails.append(tag + ("not the oracle's step", err))


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("kset", [0, 1, 2, 3, 4])
def test_ctu_invalid_cases(dev, golden, kset, fast):
    """compressible (CTU + HLLC): the staged set, the 2-d tile kernel, the row-marching kernel with
    the library's strips and with 11-row strips, and one launch per step inside comp_evolve"""
    g = golden("comp_invalid_cases")
    base = outflow_fill(ic.base_state())
    meta = cart_meta()
    s, s2 = comp_state(dev, ic.NX, ic.NY, BCS), comp_state(dev, ic.NX, ic.NY, BCS)
    fails = []
    dt0 = 0.5 * orc.comp_dt(base, ic.NX, ic.NY, NG, meta[3], meta[4], ic.GAMMA, 0.8)
    first = ic.positions()[0]
    for kind, i, j, sd, v in device_cases(g):
        tag = (kind, i, j, sd)
        U = ic.apply_case(base, kind, i, j)
        P, cfl = dev_params(meta, fast_math=fast, small_dens=sd, **kset_kw(kset))
        Po, _ = meta_to_params(meta, BCS, small_dens=sd)
        if v:
            if kset != 4:         # (a single step of 4 is a single step of 3)
                expect_rejected_step(tag, s, U, lambda: s.comp_step(P, dt0), s.comp_dt_is_cached, fails)
            if kset != 0:         # (the staged set steps from the host)
                expect_rejected_evolve(tag, s, s2, U, lambda pol, n: s.comp_evolve(P, cfl, pol, n), fails,
                                       again=(i, j) == first)
            continue
        Uo = U.copy()
        assert orc.comp_step(Uo, Po, dt0)[0] == 0
        if kset != 4:
            s.upload(U)
            s.fill_bc()
            s.comp_step(P, dt0)
            check_accepted(tag + ("step",), dev, s.download(), Uo, fast, fails)
        if kset != 0:
            # two steps of a device-side run against the oracle's (the second one is the
            # single launch of kset 4)
            Uo, pol_o = U.copy(), DtPolicy(1.e30)
            for _ in range(2):
                orc.comp_fill_bc(Uo, ic.NX, ic.NY, NG, BCS)
                dt = pol_o(orc.comp_dt(Uo, ic.NX, ic.NY, NG, meta[3], meta[4], ic.GAMMA, cfl))
                assert orc.comp_step(Uo, Po, dt)[0] == 0
                pol_o.advance(dt)
            s.upload(U)
            pol = DtPolicy(1.e30)
            s.comp_evolve(P, cfl, pol, 2)
            if pol.n != 2:
                fails.append(tag + ("evolve: steps", pol.n))
            check_accepted(tag + ("evolve",), dev, s.download(), Uo, fast, fails)
    assert not fails, report(fails)


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("path", ["rhs_staged", "rhs_wave", "step"])
def test_rk_invalid_cases(dev, golden, path, fast):
    """compressible_rk: the right-hand side by the staged kernels and by one launch of the
    row-marching kernel's method-of-lines instance, and the whole Runge-Kutta step in one call"""
    g = golden("comp_invalid_cases")
    base = outflow_fill(ic.base_state())
    meta = cart_meta()
    a, b = RK_TABLEAU["RK4"]
    s = comp_state(dev, ic.NX, ic.NY, BCS)
    kst = device.DeviceState(dev, ic.NX, ic.NY, NG, [["outflow"] * 4] * 16)
    kst.upload(np.zeros((ic.NX + 2 * NG, ic.NY + 2 * NG, 16)))
    fails = []
    dt0 = 0.3 * orc.comp_rk_dt(base, ic.NX, ic.NY, NG, meta[3], meta[4], ic.GAMMA, 0.8)
    for kind, i, j, sd, v in device_cases(g):
        tag = (kind, i, j, sd)
        U = ic.apply_case(base, kind, i, j)
        P, cfl = dev_params(meta, fast_math=fast, small_dens=sd, kernel_set=0 if path == "rhs_staged" else 2,
                            march_rows=11)
        Po, _ = meta_to_params(meta, BCS, small_dens=sd)
        if path == "step":
            assert s.comp_rk_can_fuse(P, kst, 4)
            call = lambda: s.comp_rk_step(P, kst, dt0, a, b)       # noqa: E731
        else:
            call = lambda: s.comp_rk_rhs(P, kst, 0)                # noqa: E731
        if v:
            expect_rejected_step(tag, s, U, call, s.comp_rk_dt_is_cached, fails)
            continue
        s.upload(U)
        s.fill_bc()
        call()
        if path == "step":
            Uo = U.copy()
            rk_try(Uo, Po, BCS, dt0, "RK4", inplace=True)
            check_accepted(tag, dev, s.download(), Uo, fast, fails)
        else:
            Uo = U.copy()
            rc, ko = orc.comp_rk_rhs(Uo, Po)
            assert rc == 0
            kd = kst.download()[..., 0:4]
            if fast:
                ok = np.isfinite(kd[INT]).all()
            elif dev.kind == "emu":
                ok = np.array_equal(kd[INT], ko[INT])
            else:
                ok = max(max_rel_err(kd[INT][..., n], ko[INT][..., n]) for n in range(4)) <= TOL_EXACT
            if not ok:
                fails.append(tag + ("not the oracle's right-hand side",))
    assert not fails, report(fails)


def rk_try(U, P, bcs, dt, method, inplace=False):
    """helpers.oracle_rk_step that reports: the first stage whose state the oracle rejects (-1:
    none, U advanced when inplace), and that stage's state"""
    a, b = RK_TABLEAU[method]
    ks = []
    for st in range(len(b)):
        y = U.copy()
        for jj in range(st):
            y[INT] += dt * a[st][jj] * ks[jj][INT]
        orc.comp_fill_bc(y, P.nx, P.ny, P.ng, bcs, P.gamma, P.grav, P.dy)
        y0 = y.copy()
        rc, k = orc.comp_rk_rhs(y, P)
        if rc:
            return st, y0
        if st == 0 and inplace:
            U[...] = y              # the state itself is filled and floored in place
        ks.append(k)
    if inplace:
        for st in range(len(b)):
            U[INT] += dt * b[st] * ks[st][INT]
    return -1, None


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("kset", [0, 1, 2])
def test_spherical_invalid_cases(dev, golden, kset, fast):
    """SphericalPolar grid, CGF solver: the staged set, the tile kernel, the row-marching kernel"""
    g = golden("comp_invalid_cases")
    sb, meta, bcs, geom, gs = sph_base(golden)
    nx, ny = int(meta[0]), int(meta[1])
    solid = [int(b in ("reflect", "reflect-even", "reflect-odd", "dirichlet")) for b in bcs]
    dom = gs["c0_g_domain"]
    arrays = {n: gs["c0_g_" + n] for n in SPH_NAMES}

    def state():
        st = comp_state(dev, nx, ny, bcs)
        st.set_geometry(arrays, dom[0], dom[2])
        return st
    s, s2 = state(), state()
    fails = []
    dt0 = 0.5 * orc.comp_dt_geom(sb, nx, ny, NG, geom, meta[5], meta[13])
    first = ic.sph_positions(nx, ny)[0]
    for kind, i, j, sd, v in device_cases(g, sph=True):
        tag = (kind, i, j, sd)
        U = ic.apply_case(sb, kind, i, j)
        P, cfl = dev_params(meta, kernel_set=kset, riemann="CGF", solid_xl=solid[0], solid_yl=solid[2],
                            fast_math=fast, small_dens=sd)
        Po, _ = meta_to_params(meta, bcs, riemann="CGF", small_dens=sd)
        if v:
            expect_rejected_step(tag, s, U, lambda: s.comp_step(P, dt0), s.comp_dt_is_cached, fails)
            if kset != 0:
                expect_rejected_evolve(tag, s, s2, U, lambda pol, n: s.comp_evolve(P, cfl, pol, n), fails,
                                       again=(i, j) == first)
            continue
        Uo = U.copy()
        assert orc.comp_step(Uo, Po, dt0, geom=geom)[0] == 0
        s.upload(U)
        s.fill_bc()
        s.comp_step(P, dt0)
        check_accepted(tag, dev, s.download(), Uo, fast, fails)
    assert not fails, report(fails)


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("kset", [1, 2, 3, 4])
def test_junk_in_ghost_cells_only(dev, kset, fast):
    """comp_evolve fills before it reads: NaN in every ghost cell of the upload changes nothing"""
    base = ic.base_state()
    meta = cart_meta()
    junk = np.full_like(base, np.nan)
    junk[INT] = base[INT]
    P, cfl = dev_params(meta, fast_math=fast, **kset_kw(kset))
    out = []
    for U in (base, junk):
        s = comp_state(dev, ic.NX, ic.NY, BCS)
        s.upload(U)
        pol = DtPolicy(1.e30)
        dts = list(s.comp_evolve(P, cfl, pol, 3))
        out.append((dts, s.download(), pol.n, pol.t))
    assert out[0][0] == out[1][0] and len(out[0][0]) == 3
    assert out[0][2:] == out[1][2:]
    assert same_bits(out[0][1], out[1][1])
    assert np.isfinite(out[1][1]).all()


@pytest.mark.parametrize("fast", [0, 1])
def test_pyro_class_refuses_a_nan(dev, fast, tmp_path, monkeypatch):
    """Pyro("compressible") with the problem's own parameters, on the row-marching kernel: a NaN
    written into cc_data makes single_step() and run_sim() raise, and the clock stands still"""
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    from pyro2_amd.pyro_sim import Pyro
    for call in ("single_step", "run_sim"):
        p = Pyro("compressible")
        p.initialize_problem("sedov", inputs_dict={"mesh.nx": 32, "mesh.ny": 64, "gpu.kernel_set": 2,
                                                   "gpu.fast_math": fast, "driver.max_steps": 6,
                                                   "vis.dovis": 0, "io.do_io": 0, "driver.verbose": 0})
        p.single_step()
        n0, t0 = p.sim.n, p.sim.cc_data.t
        assert n0 == 1 and t0 > 0.0
        ener = p.sim.cc_data.get_var("energy")
        ener[NG + 9, NG + 57] = np.nan
        with pytest.raises(PyroHipError) as ei:
            getattr(p, call)()
        assert ei.value.code == ERR_STATE, call
        assert p.sim.n == n0 and p.sim.cc_data.t == t0, call
        assert np.isnan(np.asarray(p.sim.cc_data.get_var("energy"))[NG + 9, NG + 57])


# ---------------------------------------------------------------------------
# a run that turns invalid inside a call
# ---------------------------------------------------------------------------
def oracle_collide(mach):
    """the colliding streams on the oracle with the driver's dt policy: states[n] = the state
    after n steps, the dts, and min(e) / max(E / rho) of the last accepted input and of the
    state the oracle rejects"""
    meta = ic.collide_meta()
    P, cfl = meta_to_params(meta, ic.COLLIDE_BCS)
    U = ic.collide_state(mach)
    pol = DtPolicy(1.e30, *ic.COLLIDE_DRV)
    states, dts, margins = [U.copy()], [], []
    while True:
        orc.comp_fill_bc(U, P.nx, P.ny, P.ng, ic.COLLIDE_BCS, P.gamma, P.grav, P.dy)
        dt = pol(orc.comp_dt(U, P.nx, P.ny, P.ng, P.dx, P.dy, P.gamma, cfl))
        margins.append(ic.margin(U))
        V = U.copy()
        if orc.comp_step(V, P, dt)[0]:
            break
        U = V
        pol.advance(dt)
        dts.append(dt)
        states.append(U.copy())
        assert pol.n < 40
    return states, dts, margins[-2:], pol


_COLLIDE = {}


def collide(golden, m):
    """... once per session, checked against the fixture (the reference's run stopped entering
    the same step after the same dts)"""
    if m not in _COLLIDE:
        g = golden("comp_invalid_cases")
        mach = ic.COLLIDE_MACH[m]
        assert float(g[f"collide{m}_mach"]) == mach
        states, dts, margins, pol = oracle_collide(mach)
        k = int(g[f"collide{m}_k"])
        assert len(dts) == k == int(g[f"collide{m}_ref_k"]) and k >= 1
        assert max_rel_err(np.array(dts), g[f"collide{m}_dts"]) <= 1e-13
        assert np.allclose(margins, g[f"collide{m}_margins"], rtol=1e-6, atol=0)
        # a condition on the INPUT: both builds stand on the same side of the assert at every
        # step (the fast build differs by 1e-10 at most)
        assert margins[0] >= 1e-6 and margins[1] <= -1e-6, margins
        _COLLIDE[m] = (states, dts, k, pol)
    return _COLLIDE[m]


def check_collide_end(tag, dev, s, pol, dts, golden, m, fast):
    states, dto, k, polo = collide(golden, m)
    assert pol.n == k, (tag, pol.n, k)
    exact_emu = dev.kind == "emu" and not fast
    assert len(dts) == k, (tag, len(dts))
    if exact_emu:
        assert list(dts) == dto, tag
        assert pol.t == polo.t
    else:
        assert max_rel_err(np.array(dts), np.array(dto)) <= 1e-12, tag
        assert abs(pol.t / polo.t - 1) <= 1e-12
    U = s.download()
    # (the emulator's exact build is the oracle bit for bit)
    tol = 0.0 if exact_emu else (TOL_FAST if fast else TOL_EXACT)
    assert_state_close(U[INT], states[k][INT], tol, fast, tag)
    # the ghost frame: the fill the failing step was entered with
    assert same_bits(U, outflow_fill(U)), (tag, "ghost frame", ndiff(U, outflow_fill(U)))
    assert not s.comp_dt_is_cached()


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("kset", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("m", [0, 1])
def test_run_turns_invalid_inside_a_call(dev, golden, m, kset, fast):
    """colliding supersonic streams (Mach 10 / 100 against each other in both directions): the
    scheme itself produces e < 0 after k good steps.  comp_evolve(k + 3): ERR_STATE after exactly
    k steps, their dts and the state after them are the oracle's, the ghost frame is that state's
    fill; the same in chunks with the failing step first in its chunk.  (The staged set, kset 0,
    steps from the host: the same loop call by call.)"""
    states, dto, k, polo = collide(golden, m)
    meta = ic.collide_meta()
    P, cfl = dev_params(meta, fast_math=fast, **kset_kw(kset))
    U0 = states[0]
    if kset == 0:
        s = comp_state(dev, ic.NX, ic.NY, BCS)
        s.upload(U0)
        pol, dts = DtPolicy(1.e30, *ic.COLLIDE_DRV), []
        with pytest.raises(PyroHipError) as ei:
            for _ in range(k + 3):
                s.fill_bc()
                dt = pol(s.comp_dt(P, cfl))
                s.comp_step(P, dt)
                pol.advance(dt)
                dts.append(dt)
        assert ei.value.code == ERR_STATE
        check_collide_end(("staged", m), dev, s, pol, dts, golden, m, fast)
        return
    for chunks in ((k + 3,), (k, 3)):
        s = comp_state(dev, ic.NX, ic.NY, BCS)
        s.upload(U0)
        pol, dts = DtPolicy(1.e30, *ic.COLLIDE_DRV), []
        with pytest.raises(PyroHipError) as ei:
            for c in chunks:
                dts += list(s.comp_evolve(P, cfl, pol, c))
        assert ei.value.code == ERR_STATE
        assert ei.value.steps_done == (k if len(chunks) == 1 else 0), (chunks, ei.value.steps_done)
        dts += list(ei.value.dts)
        check_collide_end((chunks, m, kset), dev, s, pol, dts, golden, m, fast)
        # ... and the object stays refused: nothing advances on the next call either
        with pytest.raises(PyroHipError):
            s.comp_evolve(P, cfl, pol, 2)
        assert pol.n == k


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("mach,nsteps,stage", [(10.0, 6, 3), (30.0, 3, 1)])
def test_rk_stage_turns_invalid_inside_a_step(dev, mach, nsteps, stage, fast):
    """compressible_rk, RK4 on the colliding streams: after nsteps good steps the step's own input
    is accepted and a LATER stage's state is rejected (scanned on the oracle over Mach 10 / 30 /
    100 / 300: RK4 meets one at every Mach number).  The whole-step call answers ERR_STATE and
    leaves U as it was; comp_rk_evolve stops after nsteps."""
    meta = ic.collide_meta()
    Po, cfl = meta_to_params(meta, ic.COLLIDE_BCS)
    a, b = RK_TABLEAU["RK4"]
    U = ic.collide_state(mach)
    pol = DtPolicy(1.e30, *ic.COLLIDE_DRV)
    dto = []
    while True:
        orc.comp_fill_bc(U, Po.nx, Po.ny, Po.ng, ic.COLLIDE_BCS, Po.gamma, Po.grav, Po.dy)
        dt = pol(orc.comp_rk_dt(U, Po.nx, Po.ny, Po.ng, Po.dx, Po.dy, Po.gamma, cfl))
        V = U.copy()
        st, ybad = rk_try(V, Po, ic.COLLIDE_BCS, dt, "RK4", inplace=True)
        if st >= 0:
            break
        U = V
        pol.advance(dt)
        dto.append(dt)
        assert pol.n < 40
    assert (pol.n, st) == (nsteps, stage)
    # conditions on the input: the step's own state is well inside, the rejected stage well outside
    assert ic.margin(U) >= 1e-6 and ic.margin(ybad) <= -1e-6, (ic.margin(U), ic.margin(ybad))
    P, _ = dev_params(meta, kernel_set=2, march_rows=11, fast_math=fast)
    s = comp_state(dev, ic.NX, ic.NY, BCS)
    kst = device.DeviceState(dev, ic.NX, ic.NY, NG, [["outflow"] * 4] * 16)
    s.upload(U)
    s.fill_bc()
    pre = s.download()
    assert s.comp_rk_can_fuse(P, kst, 4)
    with pytest.raises(PyroHipError) as ei:
        s.comp_rk_step(P, kst, dt, a, b)
    assert ei.value.code == ERR_STATE
    assert same_bits(s.download(), pre), ndiff(s.download(), pre)
    assert not s.comp_rk_dt_is_cached()
    # the run from the start
    s.upload(ic.collide_state(mach))
    pol_d = DtPolicy(1.e30, *ic.COLLIDE_DRV)
    with pytest.raises(PyroHipError) as ei:
        s.comp_rk_evolve(P, kst, a, b, cfl, pol_d, nsteps + 3)
    assert ei.value.code == ERR_STATE and ei.value.steps_done == nsteps and pol_d.n == nsteps
    assert max_rel_err(np.array(ei.value.dts), np.array(dto)) <= (0.0 if dev.kind == "emu" and not fast else 1e-12)
    tol = 0.0 if dev.kind == "emu" and not fast else (TOL_FAST if fast else TOL_EXACT)
    assert_state_close(s.download()[INT], U[INT], tol, fast, "rk run")
