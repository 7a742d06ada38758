"""An ensemble of small compressible runs stepped together (pyrohip_comp_evolve_batch: k_dt_policy_batch +
k_ctu_fused_batch, csrc/evolve.hip / csrc/comp_fused.hip; DeviceState.comp_evolve_batch; pyro2_amd/ensemble.py;
DESIGN.md 3.6.3).  The feature adds no physics: every member must come out exactly as from pyrohip_comp_evolve
on it alone -- a path tests/test_ctu_oracle.py and the recorded runs hold to the C oracle -- bit for bit with
gpu.fast_math = 0 (the same device code, contraction off), within the project's 1e-10 element-wise bound with
gpu.fast_math = 1 (the batch instance is another compilation).  One test goes to the oracle directly.

Shapes: 4 x 4 (one ragged tile), 14 x 30 (exactly one tile), 15 x 31 (four tiles, three nearly empty), 29 x 61
(3 x 3 ragged tiles), and on the GPU 112 x 240 (8 x 8 tiles: the XCD walk of xcd_tile in its non-identity
branch).  States: comp_scalars_cases.rough_state, one seed per member, one member with the energy jump of 10^3 on
a tile seam.  The `dev` tests run on the emulated build here and on the MI355X under -m gpu."""
import ctypes

import numpy as np
import pytest

import comp_scalars_cases as cs
import ctu_cases as cc
from conftest import comp_floors, elementwise_err, max_rel_err
from helpers import DtPolicy
from oracle import orc
from pyro2_amd import _lib, device
from test_device_compressible import TOL_EXACT, TOL_FAST, comp_state

NG = cc.NG
CFL = 0.8
GAMMA = 1.4
I = (slice(NG, -NG), slice(NG, -NG))
# the index-map boundary mixes: all-periodic, all-outflow, reflect x / periodic y, outflow x / reflect y
BCS = [("periodic",) * 4, ("outflow",) * 4, ("reflect", "reflect", "periodic", "periodic"),
       ("outflow", "outflow", "reflect", "reflect")]
# reconstruction instances: STD (limiter 2 with flattening), and the generic one (limiter 1; no flattening)
RECON = [(2, 1), (1, 1), (2, 0)]
SHAPES = [(4, 4), (14, 30), (15, 31), (29, 61)]
MEMBERS = [1, 2, 3, 9]        # 9: more members than XCDs
# (shape, N): every N at the one-tile shapes and at four tiles.  On the GPU only: 112 x 240, and 29 x 61 with nine
# members -- 81 workgroups a launch, half a minute of the single-threaded emulator for one case, where the suite's
# cases take seconds; the emulator sees nine members at one and at four tiles and 3 x 3 tiles with up to three
PAIRS = [(s, n) for s in SHAPES for n in MEMBERS if not (s == (29, 61) and n == 9)]


def rotation(shape, n):
    """solver, boundary mix and reconstruction of a (shape, N) pair, taken in turn so that the list covers
    every solver with both instances and every boundary mix (test_case_list_covers)"""
    k = (SHAPES + [(112, 240)]).index(shape) * len(MEMBERS) + MEMBERS.index(n)
    return cc.SOLVERS[k % 3], BCS[(k // 2 + k) % 4], RECON[(k // 3) % 3]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def params(shape, bcs, solver, lim, flat, fast, **kw):
    nx, ny = shape
    dx, dy = cc.spacing(nx, ny)
    Po = orc.comp_params(nx, ny, NG, dx, dy, gamma=GAMMA, limiter=lim, use_flattening=flat, bcs=tuple(bcs),
                         riemann=solver)
    kw.setdefault("kernel_set", 1)
    return device.make_comp_params(dx, dy, gamma=GAMMA, limiter=lim, use_flattening=flat, riemann=solver,
                                   solid_xl=Po.solid_xl, solid_yl=Po.solid_yl, fast_math=fast, **kw)


def member_states(shape, n, seed0=100):
    """rough states, one seed per member; the LAST member carries the Sedov-like energy jump from the first
    tile seam on (the middle of a one-tile grid)"""
    nx, ny = shape
    seam = (cc.TILE[0] if nx > cc.TILE[0] else nx // 2, cc.TILE[1] if ny > cc.TILE[1] else ny // 2)
    return [np.ascontiguousarray(cs.rough_state(nx, ny, seed0 + 17 * shape[0] + m,
                                                jump=seam if m == n - 1 else None)[0][..., :4]) for m in range(n)]


def upload_all(dev, shape, bcs, states):
    out = []
    for U in states:
        s = comp_state(dev, shape[0], shape[1], list(bcs))
        s.upload(U)
        out.append(s)
    return out


def single_runs(dev, shape, bcs, P, states, steps, tmax=None, calls=None):
    """each member alone through comp_evolve (the calls of `calls`, default one of `steps`): what a member of
    the batch must equal -- state with its ghost frame, dt sequence, policy, cached minimum, next dt"""
    out = []
    for m, U in enumerate(states):
        (s,) = upload_all(dev, shape, bcs, [U])
        pol = DtPolicy(1.e30 if tmax is None else tmax[m], 0.1)
        dts, err = [], None
        try:
            for k in (calls or [steps]):
                dts += list(s.comp_evolve(P, CFL, pol, k))
        except _lib.PyroHipError as e:
            err, dts = e, dts + list(e.dts)
        out.append(dict(U=s.download(), dts=dts, t=pol.t, n=pol.n, dt_old=pol.dt_old, cached=s.comp_dt_is_cached(),
                        next_dt=s.comp_dt(P, CFL) if err is None else None, err=err))
    return out


def compare(tag, fast, P, states, pols, dts, ref, worst, where=None):
    """members of a batch against their single runs (where: the part of the arrays compared, default all of
    them, ghost frame included); worst: [largest deviation seen]"""
    for m, (s, pol, d, r) in enumerate(zip(states, pols, dts, ref)):
        U = s.download()
        if where is not None:       # (the next dt is the minimum over the whole array, ghost cells included)
            U, r = U[where], dict(r, U=r["U"][where], next_dt=None)
        assert len(d) == len(r["dts"]) and pol.n == r["n"], (tag, m, list(d), r["dts"])
        assert s.comp_dt_is_cached() == r["cached"], (tag, m)
        if not fast:
            assert np.array_equal(bits(U), bits(r["U"])), (tag, m, np.argwhere(U != r["U"])[:5])
            assert list(d) == r["dts"] and pol.t == r["t"] and pol.dt_old == r["dt_old"], (tag, m, list(d), r["dts"])
            if r["next_dt"] is not None:
                assert s.comp_dt(P, CFL) == r["next_dt"], (tag, m)
            continue
        fl = comp_floors(r["U"], GAMMA)
        err = max(elementwise_err(U[..., k], r["U"][..., k], fl[k]) for k in range(4))
        derr = max([abs(a / b - 1.0) for a, b in zip(d, r["dts"])] + [abs(pol.t - r["t"]) / max(abs(r["t"]), 1e-300)])
        worst[0] = max(worst[0], err, derr)
        assert err <= TOL_FAST and derr <= TOL_FAST, (tag, m, err, derr)
        if r["next_dt"] is not None:
            assert abs(s.comp_dt(P, CFL) / r["next_dt"] - 1.0) <= TOL_FAST, (tag, m)


def batch_against_singles(dev, shape, n, fast, steps):
    solver, bcs, (lim, flat) = rotation(shape, n)
    P = params(shape, bcs, solver, lim, flat, fast)
    U0 = member_states(shape, n)
    ref = single_runs(dev, shape, bcs, P, U0, steps)
    states = upload_all(dev, shape, bcs, U0)
    pols = [DtPolicy(1.e30, 0.1) for _ in U0]
    dts, status = device.DeviceState.comp_evolve_batch(states, P, CFL, pols, steps)
    assert status == [0] * n and all(len(d) == steps for d in dts) and all(r["cached"] for r in ref)
    worst = [0.0]
    compare((shape, n, solver, bcs, lim, flat, fast), fast, P, states, pols, dts, ref, worst)
    if fast:
        print(f"{shape} N = {n} {solver} {bcs} limiter {lim} flattening {flat}: contracted batch against the "
              f"single runs, largest deviation {worst[0]:.3e}")
    return worst[0]


# ---------------------------------------------------------------- 1. each member equals its own single run
def test_case_list_covers():
    """a guard on this file's own case table, not on the feature (it passes without it): solver, boundary mix,
    reconstruction and N are covered by a rotation, not by their full product -- every Riemann solver with the
    STD instance and with the generic one, every boundary mix, every N at one tile and at four, every shape"""
    seen = set()
    for shape, n in PAIRS + [((29, 61), 9), ((112, 240), 3)]:
        solver, bcs, (lim, flat) = rotation(shape, n)
        seen |= {("inst", solver, lim == 2 and flat == 1), ("bc", bcs), ("n", n, shape in ((4, 4), (14, 30))),
                 ("shape", shape), ("recon", lim, flat)}
    assert all(("inst", s, std) in seen for s in cc.SOLVERS for std in (True, False))
    assert all(("bc", b) in seen for b in BCS) and all(("recon",) + r in seen for r in RECON)
    assert all(("n", n, one) in seen for n in MEMBERS for one in (True, False))
    assert all(("shape", s) in seen for s in SHAPES + [(112, 240)])


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("shape,n", PAIRS, ids=[f"{s[0]}x{s[1]}-N{n}" for s, n in PAIRS])
def test_batch_members_equal_single_runs(dev, shape, n, fast):
    """comp_evolve_batch over N members against comp_evolve on a copy of each alone, same max_steps and policy:
    all four planes with the ghost frame, the dt sequence, t, n, dt_old, steps_done; afterwards
    comp_dt_is_cached() and comp_dt().  fast_math = 0: bit for bit.  fast_math = 1: within 1e-10 element-wise
    (conftest.elementwise_err with comp_floors), the largest deviation printed"""
    batch_against_singles(dev, shape, n, fast, 4 if shape[0] * shape[1] <= 14 * 30 and n < 9 else 3)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("shape,n", [((29, 61), 9), ((112, 240), 3)], ids=["29x61-N9", "112x240-N3"])
def test_batch_members_equal_single_runs_gpu(hip, shape, n, fast):
    """the same at nine members of 3 x 3 tiles and at 112 x 240: 8 x 8 tiles, the XCD walk of xcd_tile in its
    non-identity branch"""
    assert shape != (112, 240) or (-(-shape[0] // cc.TILE[0]) * -(-shape[1] // cc.TILE[1])) % 8 == 0
    batch_against_singles(hip, shape, n, fast, 3)


# ---------------------------------------------------------------- 2. directly against the oracle
@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("solver", cc.SOLVERS)
def test_batch_against_oracle(dev, solver, fast):
    """15 x 31, three members, three steps: orc.comp_step chained under the driver's policy per member (as
    tests/test_ctu_oracle.py does for comp_evolve).  Bit-faithful build: dt lists and interiors equal on the
    emulator, within TOL_EXACT on the GPU; contracted build: within TOL_FAST = 1e-10 element-wise"""
    shape, steps = (15, 31), 3
    nx, ny = shape
    dx, dy = cc.spacing(nx, ny)
    k = cc.SOLVERS.index(solver)
    bcs, (lim, flat) = BCS[(k + 2) % 4], RECON[k % 3]
    Po = orc.comp_params(nx, ny, NG, dx, dy, gamma=GAMMA, limiter=lim, use_flattening=flat, bcs=tuple(bcs),
                         riemann=solver)
    U0 = member_states(shape, 3, seed0=500)
    oracle = []
    for U in U0:
        Uo, pol, dto = U.copy(), DtPolicy(1.e30, 0.1), []
        for _ in range(steps):
            orc.comp_fill_bc(Uo, nx, ny, NG, list(bcs), GAMMA, 0.0, dy)
            dto.append(pol(orc.comp_dt(Uo, nx, ny, NG, dx, dy, GAMMA, CFL)))
            assert orc.comp_step(Uo, Po, dto[-1])[0] == 0
            pol.advance(dto[-1])
        oracle.append((Uo, dto, pol.t))
    states = upload_all(dev, shape, bcs, U0)
    pols = [DtPolicy(1.e30, 0.1) for _ in U0]
    dts, status = device.DeviceState.comp_evolve_batch(states, params(shape, bcs, solver, lim, flat, fast), CFL,
                                                       pols, steps)
    assert status == [0, 0, 0]
    for m, (s, pol, d) in enumerate(zip(states, pols, dts)):
        U, (Uo, dto, to) = s.download(), oracle[m]
        derr = float(np.abs(np.array(d) / np.array(dto) - 1).max())
        if fast:
            fl = comp_floors(Uo[I], GAMMA)
            err = max(elementwise_err(U[I][..., v], Uo[I][..., v], fl[v]) for v in range(4))
            print(f"{solver} member {m}: contracted batch against the oracle {err:.3e}, dt {derr:.3e}")
            assert err <= TOL_FAST and derr <= TOL_FAST, (m, err, derr)
        elif dev.kind == "emu":
            assert list(d) == dto and pol.t == to, (m, list(d), dto)
            assert np.array_equal(U[I], Uo[I]), (m, np.argwhere(U[I] != Uo[I])[:5])
        else:
            err = max(max_rel_err(U[I][..., v], Uo[I][..., v]) for v in range(4))
            print(f"{solver} member {m}: batch against the oracle {err:.3e}, dt {derr:.3e}")
            assert err <= TOL_EXACT and derr <= TOL_EXACT, (m, err, derr)


# ---------------------------------------------------------------- 3. members that end at different steps
@pytest.mark.parametrize("fast", [0, 1])
def test_members_end_at_different_steps(dev, fast):
    """three members whose tmax lets them advance 1, 3 and all 5 of 5 iterations, each against its single
    comp_evolve with the same tmax; then the same members through two batch calls, 2 + 3 steps, against the
    single runs' two calls and the one call of 5: the second call starts from the cached minimum where the
    first one's last launch advanced the member, and from a full reduction where it idled"""
    shape, steps = (15, 30), 5          # two tiles
    solver, bcs, (lim, flat) = "HLLC", BCS[2], RECON[0]
    P = params(shape, bcs, solver, lim, flat, fast)
    U0 = member_states(shape, 3, seed0=900)
    # the first dt of a member is 0.1 cfl min(...) of its filled array and the policy lets it double from step to
    # step: half a first step, then 1 + 2 + half of 4 first steps (the step counts are asserted below)
    nx, ny = shape
    dx, dy = cc.spacing(nx, ny)
    dt0 = [0.1 * orc.comp_dt(orc.comp_fill_bc(U.copy(), nx, ny, NG, list(bcs), GAMMA, 0.0, dy), nx, ny, NG, dx, dy,
                             GAMMA, CFL) for U in U0]
    tmax = [0.5 * dt0[0], 5.0 * dt0[1], 1.e30]
    ref = single_runs(dev, shape, bcs, P, U0, steps, tmax=tmax)
    assert [len(r["dts"]) for r in ref] == [1, 3, 5] and [r["cached"] for r in ref] == [False, False, True]
    worst = [0.0]
    states = upload_all(dev, shape, bcs, U0)
    pols = [DtPolicy(t, 0.1) for t in tmax]
    dts, status = device.DeviceState.comp_evolve_batch(states, P, CFL, pols, steps)
    assert status == [0, 0, 0] and [len(d) for d in dts] == [1, 3, 5]
    assert pols[0].t == tmax[0] and pols[1].t == tmax[1]
    compare("one call", fast, P, states, pols, dts, ref, worst)
    # 2 + 3 steps
    ref2 = single_runs(dev, shape, bcs, P, U0, steps, tmax=tmax, calls=[2, 3])
    states = upload_all(dev, shape, bcs, U0)
    pols = [DtPolicy(t, 0.1) for t in tmax]
    da, sa = device.DeviceState.comp_evolve_batch(states, P, CFL, pols, 2)
    assert [len(d) for d in da] == [1, 2, 2] and [s.comp_dt_is_cached() for s in states] == [False, True, True]
    db, sb = device.DeviceState.comp_evolve_batch(states, P, CFL, pols, 3)
    assert sa == sb == [0, 0, 0] and [len(d) for d in db] == [0, 1, 3]
    both = [list(a) + list(b) for a, b in zip(da, db)]
    compare("2 + 3 against the single runs' 2 + 3", fast, P, states, pols, both, ref2, worst)
    # (a member that had ended before the second call has its ghost cells filled again by that call's first
    # iteration, as in a single run: against the one call of 5 the interiors are compared)
    compare("2 + 3 against 5 in one call", fast, P, states, pols, both, ref, worst, where=I)
    if fast:
        print(f"members ending at different steps: contracted batch, largest deviation {worst[0]:.3e}")


# ---------------------------------------------------------------- 4. one invalid member
@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("kind", ["energy_below_kinetic", "nan_density"])
def test_one_invalid_member(dev, kind, fast):
    """member 1 of 3 starts with one interior cell that is no gas (the contract of tests/test_invalid_state.py):
    status [0, ERR_STATE, 0]; member 1 is left as a single comp_evolve leaves it -- state, ghost cells, policy
    --, the error names it and the steps taken; members 0 and 2 equal their single runs"""
    shape, steps = (15, 30), 3          # two tiles
    solver, bcs, (lim, flat) = "CGF", BCS[3], RECON[1]
    P = params(shape, bcs, solver, lim, flat, fast)
    U0 = member_states(shape, 3, seed0=1300)
    cell = (NG + cc.TILE[0], NG + 3)        # first row of the second tile row
    if kind == "nan_density":
        U0[1][cell + (0,)] = np.nan
    else:
        U0[1][cell + (1,)] = 0.25 * (U0[1][cell + (2,)] ** 2 + U0[1][cell + (3,)] ** 2) / U0[1][cell + (0,)]
    ref = single_runs(dev, shape, bcs, P, U0, steps)
    assert ref[1]["err"] is not None and ref[1]["err"].code == _lib.ERR_STATE and ref[1]["dts"] == []
    assert ref[0]["err"] is None and ref[2]["err"] is None
    states = upload_all(dev, shape, bcs, U0)
    pols = [DtPolicy(1.e30, 0.1) for _ in U0]
    with pytest.raises(_lib.PyroHipError) as ei:
        device.DeviceState.comp_evolve_batch(states, P, CFL, pols, steps)
    e = ei.value
    assert type(e) is type(ref[1]["err"]) and e.code == _lib.ERR_STATE
    assert e.member == 1 and e.steps_done == 0 and "member 1" in str(e) and "0 steps" in str(e)
    assert e.status == [0, _lib.ERR_STATE, 0] and [len(d) for d in e.all_dts] == [steps, 0, steps]
    # the invalid member: the state before the failing step with its ghost cells filled, NaN for NaN
    U1 = states[1].download()
    assert np.array_equal(bits(U1), bits(ref[1]["U"])), np.argwhere(bits(U1) != bits(ref[1]["U"]))[:5]
    assert (pols[1].t, pols[1].n, pols[1].dt_old) == (ref[1]["t"], ref[1]["n"], ref[1]["dt_old"])
    assert not states[1].comp_dt_is_cached() and not ref[1]["cached"]
    worst = [0.0]
    keep = [0, 2]
    compare(kind, fast, P, [states[m] for m in keep], [pols[m] for m in keep], [e.all_dts[m] for m in keep],
            [ref[m] for m in keep], worst)


# ---------------------------------------------------------------- 5. refusals
def refused(states, P, steps=2, pols=None):
    pols = pols or [DtPolicy(1.e30, 0.1) for _ in states]
    with pytest.raises(_lib.PyroHipError) as ei:
        device.DeviceState.comp_evolve_batch(states, P, CFL, pols, steps)
    msg = str(ei.value).split(": ", 1)[1]
    assert msg.startswith("batch:"), msg
    assert all(p.n == 0 and p.t == 0.0 for p in pols)
    return msg


def test_refusals_c_abi(dev):
    """every refusal of pyrohip_comp_evolve_batch: an argument error whose message starts `batch:` and names
    the reason; nothing ran"""
    shape, bcs = (8, 8), BCS[1]
    nx, ny = shape
    P = params(shape, bcs, "HLLC", 2, 1, 0)
    U = member_states(shape, 1)[0]

    def fresh(shape=shape, bcs=bcs, ng=NG, ctx=dev):
        s = device.DeviceState(ctx, shape[0], shape[1], ng, [list(r) for r in orc.comp_var_bcs(bcs)])
        return s
    a, b = fresh(), fresh()
    for s in (a, b):
        s.upload(U)
    other = device.Context(0)
    elsewhere = fresh(ctx=other)
    assert "context" in refused([a, elsewhere], P)
    del elsewhere
    other.close()
    assert "shape" in refused([a, fresh(shape=(8, 9))], P)
    assert "ng" in refused([a, fresh(ng=5)], P)
    assert "boundary codes" in refused([a, fresh(bcs=BCS[0])], P)
    assert "twice" in refused([a, b, a], P)
    five = device.DeviceState(dev, nx, ny, NG, [list(r) for r in orc.comp_var_bcs(bcs)] + [list(orc.comp_var_bcs(bcs)[0])])
    assert "nvar" in refused([five], P) and "passive scalars" in refused([five], P)
    assert "gravity" in refused([a, b], params(shape, bcs, "HLLC", 2, 1, 0, grav=-1.0))
    h = fresh()
    h.set_heating(np.ones((h.qx, h.qy)))
    assert "heating" in refused([a, h], P)
    src, hs = fresh(), fresh()
    hs.set_source(0, src)
    assert "host-evaluated sources" in refused([a, hs], P)
    for side in ("hse", "ambient", "ramp"):
        rows = [["outflow", "outflow", "outflow", side] for _ in range(4)]
        u = device.DeviceState(dev, nx, ny, NG, rows)
        assert "hse / ambient / ramp" in refused([u], P), side
    import sph_cases as sc
    sp = fresh()
    g = sc.grid_of(nx, ny)
    sp.set_geometry(g.device_geometry(), g.xmin, g.ymin)
    assert "SphericalPolar" in refused([a, sp], P)
    slab = fresh()
    slab.set_neighbours(0, 0)
    assert "slabs" in refused([a, slab], P)
    if dev.kind == "emu":
        # (a context reduces its CFL minimum over the ranks once it has a communicator: the emulated backend's
        # hook stands for one, test_device_compressible.py::test_comp_evolve_global_minimum_every_step; the
        # check is host code, the same in both builds)
        hook = _lib.lib().pyrohip_emu_set_peer_min
        hook.argtypes, hook.restype = [ctypes.c_double], ctypes.c_int
        try:
            hook(1.0e-5)
            dev.comm_set_global_dt(True)
            assert "global CFL" in refused([a, b], P)
        finally:
            dev.comm_set_global_dt(False)
            hook(-1.0)
    for ks in (0, 2):
        assert "kernel_set 0 and 2" in refused([a, b], params(shape, bcs, "HLLC", 2, 1, 0, kernel_set=ks))
    assert "sponge" in refused([a, b], params(shape, bcs, "HLLC", 2, 1, 0, sponge=(0.1, 0.01, 0.01)))
    assert "well_balanced" in refused([a, b], params(shape, bcs, "HLLC", 2, 1, 0, well_balanced=1))
    # (a grid is at least as wide as its ghost frame: fewer than 4 cells means ng = 3)
    assert "at least 4 cells" in refused([fresh(shape=(3, 8), ng=3)], params((3, 8), bcs, "HLLC", 2, 1, 0))
    assert "at least 4 cells" in refused([fresh(shape=(8, 3), ng=3)], params((8, 3), bcs, "HLLC", 2, 1, 0))
    assert "ng >= 4" in refused([fresh(ng=3)], P)
    # ... and the two members are as good as ever
    dts, status = device.DeviceState.comp_evolve_batch([a, b], P, CFL, [DtPolicy(1.e30, 0.1) for _ in range(2)], 2)
    assert status == [0, 0] and [len(d) for d in dts] == [2, 2]


# ---------------------------------------------------------------- 6. Ensemble
def pyro_inputs(problem, fast, vary):
    if problem == "sedov":
        d = {"mesh.nx": 32, "mesh.ny": 32, "driver.max_steps": 6, "sedov.r_init": vary}
    else:
        d = {"mesh.nx": 16, "mesh.ny": 16, "driver.max_steps": 6, "kh.u_1": vary}
    d.update({"gpu.fast_math": fast, "io.do_io": 0, "vis.dovis": 0, "driver.verbose": 0})
    return d


VARY = {"sedov": (0.05, 0.1, 0.2), "kh": (-0.5, -0.3, -0.8)}


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("problem", ["sedov", "kh"])
def test_ensemble_equals_separate_pyro_runs(dev, problem, fast, monkeypatch, tmp_path):
    """three `sedov` members at 32^2 with different sedov.r_init (three `kh` members at 16 x 16, periodic, with
    different kh.u_1 -- the problem's name for the velocity of layer 1), driver.max_steps = 6, against three
    separate Pyro.run_sim() runs: cc_data.data (fast_math = 0: np.array_equal), t, n, dt"""
    from pyro2_amd.ensemble import Ensemble
    from pyro2_amd.pyro_sim import Pyro
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    inputs = "inputs." + problem
    ens = Ensemble("compressible")
    for v in VARY[problem]:
        p = ens.add(problem, inputs, pyro_inputs(problem, fast, v))
        assert isinstance(p, Pyro) and p.sim.n == 0
    assert ens.run_sim() is ens.members
    for v, member in zip(VARY[problem], ens.members):
        p = Pyro("compressible")
        p.initialize_problem(problem, inputs_file=inputs, inputs_dict=pyro_inputs(problem, fast, v))
        p.run_sim()
        a, b = member.sim, p.sim
        assert a.n == b.n == 6 and a.finished()
        A, B = np.array(a.cc_data.data), np.array(b.cc_data.data)
        if not fast:
            assert np.array_equal(bits(A), bits(B)), (v, np.argwhere(A != B)[:5])
            assert (a.cc_data.t, a.dt, a.dt_old) == (b.cc_data.t, b.dt, b.dt_old), v
        else:
            fl = comp_floors(B, GAMMA)
            err = max(elementwise_err(A[..., k], B[..., k], fl[k]) for k in range(4))
            print(f"{problem} {v}: contracted ensemble member against its Pyro run {err:.3e}")
            assert err <= TOL_FAST and abs(a.cc_data.t / b.cc_data.t - 1) <= TOL_FAST and abs(a.dt / b.dt - 1) <= TOL_FAST


def test_ensemble_members_with_their_own_tmax(dev, monkeypatch, tmp_path):
    """members that end at their own driver.tmax / driver.max_steps: every one as after its own run"""
    from pyro2_amd.ensemble import Ensemble
    from pyro2_amd.pyro_sim import Pyro
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    over = [{"driver.max_steps": 2}, {"driver.tmax": 1.e-4}, {}]
    ens = Ensemble()
    for o in over:
        ens.add("sedov", "inputs.sedov", dict(pyro_inputs("sedov", 0, 0.1), **o))
    ens.run_sim()
    assert ens.members[0].sim.n == 2 and ens.members[1].sim.cc_data.t == 1.e-4 and ens.members[2].sim.n == 6
    for o, member in zip(over, ens.members):
        p = Pyro("compressible")
        p.initialize_problem("sedov", inputs_file="inputs.sedov", inputs_dict=dict(pyro_inputs("sedov", 0, 0.1), **o))
        p.run_sim()
        assert np.array_equal(bits(np.array(member.sim.cc_data.data)), bits(np.array(p.sim.cc_data.data))), o
        assert (member.sim.cc_data.t, member.sim.n, member.sim.dt) == (p.sim.cc_data.t, p.sim.n, p.sim.dt), o


def test_ensemble_refusals(dev, monkeypatch, tmp_path, capsys):
    """every condition of Ensemble.run_sim() is refused with msg.fail, naming the first member and the option"""
    from pyro2_amd.ensemble import Ensemble
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    base = dict(pyro_inputs("sedov", 0, 0.1), **{"mesh.nx": 8, "mesh.ny": 8})

    def fails(second, *words, solver="compressible", problem="sedov", inputs="inputs.sedov"):
        ens = Ensemble(solver)
        ens.add(problem, inputs, dict(base) if solver == "compressible" else second)
        if solver == "compressible":
            ens.add(problem, inputs, dict(base, **second))
        capsys.readouterr()
        with pytest.raises(SystemExit):
            ens.run_sim()
        out = capsys.readouterr().out
        for w in words:
            assert w in out, (w, out)
        assert all(p.sim.n == 0 for p in ens.members)

    fails({"mesh.nx": 8, "mesh.ny": 8, "driver.max_steps": 2, "io.do_io": 0, "vis.dovis": 0, "driver.verbose": 0},
          "compressible_rk", "compressible solver only", solver="compressible_rk")
    fails({"gpu.kernel_set": 0}, "member 1", "can_evolve_many")
    fails({"mesh.nx": 12}, "member 1", "mesh.nx")
    fails({"mesh.xmax": 2.0}, "member 1", "mesh.xmax")
    fails({"mesh.yrboundary": "reflect"}, "member 1", "mesh.yrboundary")
    fails({"driver.cfl": 0.5}, "member 1", "driver.cfl")
    fails({"eos.gamma": 1.6}, "member 1", "gamma")
    fails({"compressible.limiter": 1}, "member 1", "limiter")
    fails({"particles.do_particles": 1}, "member 1", "particles")
    fails({"io.do_io": 1}, "member 1", "io.do_io")
    fails({"vis.dovis": 1}, "member 1", "vis.dovis")


def test_ensemble_command_line(dev, monkeypatch, tmp_path, capsys):
    """python -m pyro2_amd.ensemble compressible sedov inputs.sedov --vary sedov.r_init=... key=value: runs and
    prints one line per member (t, n, last dt)"""
    from pyro2_amd import ensemble
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    capsys.readouterr()
    ens = ensemble.main(["compressible", "sedov", "inputs.sedov", "--vary", "sedov.r_init=0.05,0.1,0.2",
                         "mesh.nx=16", "mesh.ny=16", "driver.max_steps=3", "gpu.fast_math=0"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("member ")]
    assert len(lines) == 3 and len(ens.members) == 3
    for m, (ln, p) in enumerate(zip(lines, ens.members)):
        assert ln.startswith(f"member {m} sedov.r_init=") and "n = 3" in ln and "t = " in ln and "dt = " in ln
        assert p.sim.n == 3 and p.rp.get_param("mesh.nx") == 16
    assert len({ln.split("t = ")[1] for ln in lines}) == 3         # three different runs
