"""The shallow-water kernels -- the five staged kernels, the one-launch kernel k_sw_wave in its
bit-faithful and contracted builds, the device-side stepping loop (csrc/swe.hip) -- against the
C oracle orc_swe_step (oracle/pyro_oracle.c, pinned to the reference by
tests/test_oracle_golden.py) at the seams of the launch geometry and at the scheme's edge states.

Shapes and states: tests/swe_cases.py.  Every path of k_sw_wave's unit decoding is reached for 4
compute units (the emulated device) and for 256 (the MI355X); the list is held to the library's
own geometry call, so a change of sww_rows that drops a path fails here.  The states cover the
whole array with ghost cells that are not boundary-consistent: smooth, supercritical in both
directions, +0 / -0 momenta and exactly critical cells, near-dry cells, and piecewise-constant
blocks whose jumps sit on the strip seams (with limiter 0 and HLLC: negative face heights).

The `dev` tests run on the emulated build here (bit for bit) and on the MI355X under -m gpu."""
import numpy as np
import pytest

import swe_cases as sc
from helpers import DtPolicy
from oracle import orc
from test_oracle_golden import oracle_swe_run

NG = sc.NG
TOL = 1e-13                                  # bit-faithful build on the GPU, per step (tests/test_swe.py)
FAST_TOL = 1e-10                             # contracted build, element-wise ...
FLOOR = np.array([1.0, 0.1, 0.1, 0.1])       # ... with these floors (test_swe_contracted_build_within_1e10)
CFL = 0.8
I = (slice(NG, -NG), slice(NG, -NG))


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def geometries(shape):
    from pyro2_amd import device
    return {cus: device.swe_wave_geometry(shape[0], shape[1], NG, cus) for cus in (4, 256)}


def case_state(shape, kind):
    """(U0, dx, dy, g) of a case; the library in use gives the row seams for `blocks`"""
    nx, ny = shape
    dx, dy, g = sc.shape_params(shape)
    seams = sc.row_seams(nx, geometries(shape).values()) if kind == "blocks" else ()
    return sc.make_state(kind, nx, ny, g, sc.state_seed(shape, kind), seams), dx, dy, g


def oracle_case(shape, kind, riemann, lim):
    """one oracle step of a case: (U0, U1, dt, counts, params)"""
    U0, dx, dy, g = case_state(shape, kind)
    P = orc.swe_params(shape[0], shape[1], NG, dx, dy, g, lim, riemann)
    dt = orc.swe_dt(U0, P, CFL)
    U1 = U0.copy()
    _, counts = orc.swe_step(U1, P, dt, counts=True)
    return U0, U1, dt, counts, P


def fast_err(a, b):
    return float((np.abs(a - b) / (np.abs(b) + FLOOR)).max())


# ---------------------------------------------------------------- the case list itself
def test_wave_geometry_reaches_every_path(dev):
    """no launch: the shapes of swe_cases.PATHS take the path they are listed under, for 4 and for
    256 compute units, by the geometry the step itself goes by (pyrohip_swe_wave_geometry); the
    regular path's short last strip has the 1 and 7 rows the names say; the mixed path has both
    kinds of column strips; and the column counts sit around the strips and blocks they are for"""
    for path, by_cus in sc.PATHS.items():
        for cus, shapes in by_cus.items():
            assert shapes
            for shape in shapes:
                assert shape == sc.BIG or shape in sc.SHAPES
                geo = geometries(shape)[cus]
                name, regular, cut = sc.path_of(geo, shape[0])
                assert name == path, (shape, cus, geo)
                assert geo["col_strips"] == -(-shape[1] // sc.SWW_OUT)
                assert geo["wavefronts"] == geo["col_strips"] * geo["row_strips"] + geo["n_extra"]
                if path == "single_chunk":
                    assert shape[0] <= 16 and geo["rows_per_strip"] == shape[0]
                if path.startswith("two_regular"):
                    assert regular == [(0, 16), (16, shape[0])]
                if path == "all_cut":
                    assert geo["n_extra"] == geo["col_strips"] and min(b - a for a, b in cut) >= 8
                if path == "cut_and_regular":
                    assert 0 < geo["n_extra"] < geo["col_strips"] and geo["row_strips"] >= 2
                    assert geo["wavefronts"] == geo["slots"]
    nys = {ny for _, ny in sc.SHAPES}
    assert {57, 58, 59, 116, 117} <= nys          # full and ragged last column strips
    assert {254, 255, 257} <= nys                 # the staged kernels' second 256-thread block: ny + 2 > 256
    assert min(min(s) for s in sc.SHAPES) >= 4
    assert sc.PARAMS == [(1.3, 1.0), (0.7, 2.0)]
    assert {sc.shape_params(s)[2] for s in sc.SHAPES} == {1.0, 2.0}


COUNTERS = {"HLLC": ("hllc_exit", "shock_l", "shock_r", "h_l_nonpos", "h_r_nonpos", "e_val"),
            "Roe": ("hh_fix0", "hh_fix2", "e_val")}     # (a non-positive height is a NaN in riemann_roe: not in the list)


def test_case_list_conditions(dev):
    """the oracle alone, over the whole finite list: every result is finite; every step moves the
    interior by more than 1e-3; `blocks` with HLLC and limiter 0 has faces of negative height in
    both directions, with limiters 1 and 2 none; over the list every counter of orc.swe_step is
    non-zero for the solver it belongs to -- every HLLC exit, both shock forms, non-positive
    heights on either side of an HLLC face, both rewritten Roe wave speeds, every sign class of the tracing's
    e_val.  Two classes cannot occur in a finite state and must stay empty: e_val[0] = u - c and
    e_val[2] = u + c are -0 only for u = -0 and c = -+0, that is h = 0, where u = m / h is not
    finite.  The cases in_finite_list() leaves out are non-finite in the oracle"""
    total = {rs: {k: np.zeros((2, 12) if k == "e_val" else (2, 4) if k == "hllc_exit" else (2, 1), dtype=np.int64)
                  for k in COUNTERS[rs]} for rs in sc.SOLVERS}
    for shape in sc.SHAPES:
        for kind in sc.STATES:
            for rs in sc.SOLVERS:
                for lim in sc.LIMITERS:
                    U0, U1, dt, counts, _ = oracle_case(shape, kind, rs, lim)
                    if not sc.in_finite_list(shape, kind, rs, lim):
                        assert not np.isfinite(U1[I]).all(), (shape, kind, rs, lim)
                        continue
                    assert np.isfinite(U1).all(), (shape, kind, rs, lim)
                    assert np.abs(U1[I] - U0[I]).max() > 1e-3, (shape, kind, rs, lim)
                    neg = [c["h_l_nonpos"] + c["h_r_nonpos"] for c in counts]
                    if kind == "blocks":
                        assert (min(neg) > 0) if lim == 0 else (max(neg) == 0), (shape, rs, lim, neg)
                    for d in range(2):
                        for k in COUNTERS[rs]:
                            total[rs][k][d] += np.array(counts[d][k]).ravel()
    for rs in sc.SOLVERS:
        for k in COUNTERS[rs]:
            t = total[rs][k]
            if k == "e_val":
                impossible = np.zeros(12, dtype=bool)
                impossible[[3, 11]] = True                # -0 of e_val[0] and of e_val[2]
                assert (t[:, ~impossible] > 0).all() and (t[:, impossible] == 0).all(), (rs, t)
            else:
                assert (t > 0).all(), (rs, k, t)


# ---------------------------------------------------------------- one step
def step_checks(ctx, shape, kinds=sc.STATES, combos=None, report=None):
    """every (state, solver, limiter) of the finite list on one shape: dt, the staged step, the
    one-launch step, a second call of each, the contracted one-launch step"""
    from pyro2_amd import device
    nx, ny = shape
    exact = ctx.kind == "emu"
    s = device.DeviceState(ctx, nx, ny, NG, [["outflow"] * 4] * 4)
    for kind in kinds:
        for rs in sc.SOLVERS:
            for lim in sc.LIMITERS:
                if not sc.in_finite_list(shape, kind, rs, lim) or (combos and (kind, rs, lim) not in combos):
                    continue
                U0, Uo, dt, counts, P = oracle_case(shape, kind, rs, lim)
                tag = (shape, kind, rs, lim)
                s.upload(U0)
                dtd = s.swe_dt(P.dx, P.dy, P.g, CFL)
                assert dtd == dt if exact else abs(dtd / dt - 1) <= 1e-12, tag

                def run(ks, fast):
                    s.upload(U0)
                    s.swe_step(P.dx, P.dy, P.g, lim, rs, dt, kernel_set=ks, fast_math=fast)
                    return s.download()
                staged = run(0, 0)
                err = float(np.abs(staged[I] - Uo[I]).max())
                ghost = np.ones(U0.shape[:2], dtype=bool)
                ghost[I] = False
                assert np.array_equal(bits(staged)[ghost], bits(U0)[ghost]), tag
                wave = run(1, 0)
                fast = run(1, 1)
                ferr = fast_err(fast[I], Uo[I])
                if report is not None:
                    report.append((shape, kind, rs, lim, err, ferr))
                print(f"{nx}x{ny} {kind} {rs} limiter {lim}: staged abs err {err:.3e}, contracted {ferr:.3e}")
                assert err <= (0.0 if exact else TOL * max(1.0, np.abs(Uo[I]).max())), (tag, err)
                assert np.array_equal(wave, staged), tag
                assert np.array_equal(bits(wave)[ghost], bits(U0)[ghost]), tag
                assert np.array_equal(bits(run(1, 0)), bits(wave)), tag       # the same input again: the same bits
                assert np.array_equal(bits(run(0, 0)), bits(staged)), tag
                assert np.array_equal(bits(run(1, 1)), bits(fast)), tag
                assert np.array_equal(bits(fast)[ghost], bits(U0)[ghost]), tag
                assert ferr <= FAST_TOL, (tag, ferr)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=[f"{a}x{b}" for a, b in sc.SHAPES])
def test_swe_step_vs_oracle(dev, shape):
    """one step of every state, solver and limiter of the finite list: pyrohip_swe_dt against
    orc.swe_dt (bit for bit on the emulator, 1e-12 relative on the GPU); the staged kernels against
    the oracle over the interior (exact on the emulator, <= 1e-13 max(1, max |oracle|) on the GPU),
    the ghost cells keeping their input bits; the bit-faithful one-launch kernel equal to the
    staged kernels on the whole array; a second call from the same input giving the same bits;
    the contracted one-launch kernel element-wise <= 1e-10 of the oracle (floors 1, 0.1, 0.1, 0.1)
    -- `blocks` with HLLC and limiter 0, whose faces of negative height have a NaN wave speed in
    the reference, included"""
    step_checks(dev, shape)


@pytest.mark.gpu
def test_swe_step_vs_oracle_mixed_strips_256_cus(hip):
    """816 x 2320: on 256 compute units 8 of the 40 column strips are cut into 52 row strips, the
    other 32 into 51 regular ones (test_wave_geometry_reaches_every_path)"""
    step_checks(hip, sc.BIG, combos={("blocks", "HLLC", 1), ("zeros", "Roe", 2), ("super", "HLLC", 0)})


@pytest.mark.parametrize("shape", [(17, 61), (21, 117)], ids=["17x61", "21x117"])
def test_swe_nan_pattern_at_exact_criticality(dev, shape):
    """a uniform, exactly critical block (u = sqrt(g h) to the bit): the reference's Harten-Hyman
    fix is 0 * x / 0 there and the Roe step returns NaN around it.  The bit-faithful builds only:
    the NaN pattern and every finite value against the oracle; one-launch == staged incl. the NaNs"""
    from pyro2_amd import device
    nx, ny = shape
    U0, dx, dy, g = case_state(shape, "critical")
    s = device.DeviceState(dev, nx, ny, NG, [["outflow"] * 4] * 4)
    for lim in sc.LIMITERS:
        P = orc.swe_params(nx, ny, NG, dx, dy, g, lim, "Roe")
        dt = orc.swe_dt(U0, P, CFL)
        Uo = U0.copy()
        orc.swe_step(Uo, P, dt)
        nan = np.isnan(Uo)
        assert nan[I].any() and not nan[I].all() and np.isfinite(Uo[~nan]).all()
        out = []
        for ks in (0, 1):
            s.upload(U0)
            s.swe_step(dx, dy, g, lim, "Roe", dt, kernel_set=ks)
            out.append(s.download())
        assert np.array_equal(np.isnan(out[0]), nan), lim
        fin = ~nan
        fin[:NG], fin[-NG:], fin[:, :NG], fin[:, -NG:] = False, False, False, False
        err = np.abs(out[0][fin] - Uo[fin]).max()
        assert err <= (0.0 if dev.kind == "emu" else TOL * max(1.0, np.abs(Uo[fin]).max())), (lim, err)
        assert np.array_equal(out[0], out[1], equal_nan=True), lim


# ---------------------------------------------------------------- three steps, ghost fill in between
BCS = [("outflow", "outflow", "reflect", "reflect"), ("reflect", "reflect", "periodic", "periodic"),
       ("periodic", "periodic", "outflow", "outflow"), ("reflect", "reflect", "reflect", "reflect")]
NSTEPS = 3


def var_rows(bcs):
    vb = orc.comp_var_bcs(list(bcs))
    return [list(vb[0]), list(vb[2]), list(vb[3]), list(vb[0])]


def three_step_solvers(shape, kind):
    """`zeros`: both solvers.  `blocks`: HLLC, and Roe at 17 x 61; at 21 x 117 the reference's own Roe
    run turns NaN within the three steps (boundary-filled piecewise-constant data hands riemann_roe
    bit-equal states next to a wave speed within its tol of zero: 0 * x / 0, interface.py:353-362;
    test_swe_three_steps_vs_oracle asserts that it does) -- out of the issue's scope"""
    if kind == "zeros" or tuple(shape) == (17, 61):
        return sc.SOLVERS
    return ("HLLC",)


def three_steps(dev, shape, bcs, kind, rs, ks, fast, dto):
    """three steps on the device, dt from the device (held to the oracle's: bit for bit on the emulator,
    1e-12 relative per step on the GPU for the bit-faithful builds -- the figure of the one-step
    check; the contracted build's dt comes from its own state, 1e-10 per step)"""
    from pyro2_amd import device
    nx, ny = shape
    U0, dx, dy, g = case_state(shape, kind)
    exact = dev.kind == "emu"
    s = device.DeviceState(dev, nx, ny, NG, var_rows(bcs))
    s.upload(U0)
    pol = DtPolicy(1.e30, 0.5)
    for n in range(NSTEPS):
        s.fill_bc()
        dt = pol(s.swe_dt(dx, dy, g, CFL))
        if fast:
            assert abs(dt / dto[n] - 1) <= (n + 1) * FAST_TOL, (rs, ks, fast, n)
        else:
            assert dt == dto[n] if exact else abs(dt / dto[n] - 1) <= (n + 1) * 1e-12, (rs, ks, fast, n)
        s.swe_step(dx, dy, g, 2, rs, dt, kernel_set=ks, fast_math=fast)
        pol.advance(dt)
    return s.download()


def contracted_roe_blocks(shape, kind, rs):
    return kind == "blocks" and rs == "Roe" and tuple(shape) == (17, 61)


@pytest.mark.parametrize("kind", ["zeros", "blocks"])
@pytest.mark.parametrize("bcs", BCS, ids=["-".join(b[::2]) for b in BCS])
@pytest.mark.parametrize("shape", [(17, 61), (21, 117)], ids=["17x61", "21x117"])
def test_swe_three_steps_vs_oracle(dev, shape, bcs, kind):
    """three steps with limiter 2: ghost fill between the steps, dt from the device, against
    oracle_swe_run -- staged, one-launch and contracted kernels, the per-step tolerances times
    the step count (the contracted Roe solver on `blocks` at 17 x 61 has a test of its own below).
    And the sign of every exactly-zero momentum of the final state is the oracle's (the
    bit-faithful quotient of hydro.h turns -0 / h into +0: sw_vel undoes that for the primitive
    variables, sw_cons_flux, sw_roe and sw_hllc divide momenta by h as well).  On the emulator the
    zeros are the oracle's zeros; on the GPU, where the bit-faithful build is held to 3e-13 and not
    to the bit, a momentum that is zero on one side only must be within that bound of zero, and
    the signs are compared where both are zero"""
    nx, ny = shape
    U0, dx, dy, g = case_state(shape, kind)
    exact = dev.kind == "emu"
    for rs in sc.SOLVERS:
        P = orc.swe_params(nx, ny, NG, dx, dy, g, 2, rs)
        Uo, dto, _ = oracle_swe_run(U0, P, CFL, list(bcs), NSTEPS, f0=0.5)
        if rs not in three_step_solvers(shape, kind):
            assert not np.isfinite(Uo[I]).all(), (rs, "left out as NaN in the reference, but the oracle is finite")
            continue
        assert np.isfinite(Uo).all() and np.abs(Uo[I] - U0[I]).max() > 1e-3
        zo = Uo[I][..., 1:3] == 0.0
        if kind == "zeros":
            assert zo.sum() > 20, "the still band must leave exact zeros to compare"
        for ks, fast in ((0, 0), (1, 0), (1, 1)):
            if fast and contracted_roe_blocks(shape, kind, rs):
                continue
            U = three_steps(dev, shape, bcs, kind, rs, ks, fast, dto)
            tag = (rs, ks, fast)
            if fast:
                err = fast_err(U[I], Uo[I])
                print(shape, kind, bcs, tag, "contracted err", err)
                assert err <= NSTEPS * FAST_TOL, (tag, err)
                continue
            err = float(np.abs(U[I] - Uo[I]).max())
            print(shape, kind, bcs, tag, "abs err", err)
            bound = 0.0 if exact else NSTEPS * TOL * max(1.0, np.abs(Uo[I]).max())
            assert err <= bound, (tag, err)
            md, mo = U[I][..., 1:3], Uo[I][..., 1:3]
            zd = md == 0.0
            assert np.abs(md[zo & ~zd]).max(initial=0.0) <= bound and np.abs(mo[zd & ~zo]).max(initial=0.0) <= bound, tag
            both = zd & zo
            if kind == "zeros":
                assert both.sum() > 20, tag
            assert np.array_equal(np.signbit(md[both]), np.signbit(mo[both])), tag


@pytest.mark.parametrize("bcs", BCS, ids=["-".join(b[::2]) for b in BCS])
def test_swe_three_steps_contracted_roe_on_blocks(dev, request, bcs):
    """The contracted Roe solver on `blocks` at 17 x 61, three steps with limiter 2: 1.1e-3 .. 1.4e-3
    element-wise from the oracle on the emulator, against 3e-10, from the second step on.  Cause: the
    first step leaves the still block around cell (6, 23) with momenta that are round-off residues
    (-2.0e-17, 1.0e-17 in the oracle), and the tracing sends the transverse waves by
    copysign(1, u) (interface.py:191-193): the sign of a residue picks the face.  The contracted
    build has other residues.  No quotient is at fault and no form of the contracted arithmetic
    can reproduce the reference's last bit; the reference's own answer moves as much when the
    residues change sign (test_oracle_roe_blocks_second_step_turns_on_residues).  Kept failing,
    strictly, on the emulator.  On the MI355X the contracted build's residues come out with the
    oracle's signs and the run is within the bound (7.9e-14 .. 7.2e-13 measured; the kernels are
    deterministic, test_swe_step_vs_oracle): there the assertion simply holds."""
    shape, kind, rs = (17, 61), "blocks", "Roe"
    if dev.kind == "emu":
        request.applymarker(pytest.mark.xfail(strict=True, reason="the sign of a round-off residue of a still block's "
                                              "momentum decides the tracing's branch in the reference"))
    U0, dx, dy, g = case_state(shape, kind)
    P = orc.swe_params(shape[0], shape[1], NG, dx, dy, g, 2, rs)
    Uo, dto, _ = oracle_swe_run(U0, P, CFL, list(bcs), NSTEPS, f0=0.5)
    assert np.isfinite(Uo).all()
    U = three_steps(dev, shape, bcs, kind, rs, 1, 1, dto)
    err = fast_err(U[I], Uo[I])
    print(shape, kind, bcs, "contracted Roe err", err)
    assert err <= NSTEPS * FAST_TOL, err


def test_oracle_roe_blocks_second_step_turns_on_residues(dev):
    """what test_swe_three_steps_contracted_roe_on_blocks fails on, in the oracle alone: after one
    step of the 17 x 61 `blocks` run the only momenta below 1e-14 that are not zero sit in one cell
    of a still block; the second step from that state, and from the same state with the sign of
    those residues changed, differ by more than 1e-4"""
    shape = (17, 61)
    U0, dx, dy, g = case_state(shape, "blocks")
    P = orc.swe_params(shape[0], shape[1], NG, dx, dy, g, 2, "Roe")
    bcs = list(BCS[0])
    U1, _, _ = oracle_swe_run(U0, P, CFL, bcs, 1, f0=0.5)
    from test_oracle_golden import swe_fill
    swe_fill(U1, P, bcs)
    m = U1[..., 1:3]
    res = (np.abs(m) < 1e-14) & (m != 0.0)
    assert 0 < res.sum() <= 4 and len({(i, j) for i, j, _ in np.argwhere(res)}) == 1
    dt = orc.swe_dt(U1, P, CFL)
    A, B = U1.copy(), U1.copy()
    B[..., 1:3][res] *= -1.0
    orc.swe_step(A, P, dt)
    orc.swe_step(B, P, dt)
    assert np.isfinite(A).all() and np.isfinite(B).all()
    assert np.abs(A - B)[I].max() > 1e-4


# ---------------------------------------------------------------- the device-side loop
@pytest.mark.parametrize("lim", [0, 2])
@pytest.mark.parametrize("shape", [(17, 61), (21, 117)], ids=["17x61", "21x117"])
def test_swe_evolve_equals_single_steps_short_strips(dev, shape, lim):
    """pyrohip_swe_evolve with HLLC on grids whose second row strip has 1 and 5 rows (the step
    kernel's CFL partials of such strips feed the next dt) against the same steps taken singly:
    dt list, t, n and the whole array, both builds"""
    from pyro2_amd import device
    nx, ny = shape
    U0, dx, dy, g = case_state(shape, "smooth")
    rows = var_rows(("outflow", "outflow", "reflect", "reflect"))
    for fast in (0, 1):
        s1 = device.DeviceState(dev, nx, ny, NG, rows)
        s1.upload(U0)
        pol1, d1 = DtPolicy(1.e30), []
        for _ in range(5):
            s1.fill_bc()
            dt = pol1(s1.swe_dt(dx, dy, g, CFL))
            s1.swe_step(dx, dy, g, lim, "HLLC", dt, kernel_set=1, fast_math=fast)
            pol1.advance(dt)
            d1.append(dt)
        s = device.DeviceState(dev, nx, ny, NG, rows)
        s.upload(U0)
        pol = DtPolicy(1.e30)
        dts = list(s.swe_evolve(dx, dy, g, lim, "HLLC", CFL, pol, 2, fast_math=fast))
        dts += list(s.swe_evolve(dx, dy, g, lim, "HLLC", CFL, pol, 3, fast_math=fast))
        assert dts == d1 and pol.t == pol1.t and pol.n == pol1.n, (fast, dts, d1)
        assert np.array_equal(s.download(), s1.download()), fast
