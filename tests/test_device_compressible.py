"""HIP compressible (CTU + HLLC) step vs the reference's stage dumps, its
golden files and the oracle.

Tolerance: north_star asks 1e-10 rtol.  exact build (fast_math=0, no FMA
contraction, reference operation order): bit-identical on the emulated
backend, <= 1e-13 per step on the GPU (TOL_EXACT; the only expected source of
difference is libm pow in the rare two-rarefaction branch).  fast build
(fast_math=1): <= 1e-10 (TOL_FAST), ELEMENT-WISE: |a - b| <= 1e-10 (|b| + floor_n)
with floor_n the ambient scale of variable n (conftest.elementwise_err) -- the
array-wide max_rel_err is only used for the bit-faithful build, whose errors
are at round-off.

The fast build's reciprocal / rsqrt intrinsics and FMA contraction exist on the
GPU only (hydro.h `#if PYRO_FAST && !defined(PYRO_EMU)`): the CPU suite runs the
fast build's CODE PATHS with true divisions (test_comp_fast_path_logic), every
test of its ARITHMETIC is marked gpu.
"""


def assert_state_close(U, ref, tol, fast, what=""):
    """bit-faithful build: array-wide relative error; fast build: element-wise"""
    if fast:
        fl = comp_floors(ref)
        for n in range(4):
            e = elementwise_err(U[..., n], ref[..., n], fl[n])
            assert e <= tol, (what, "element-wise", n, e)
    else:
        for n in range(4):
            assert max_rel_err(U[..., n], ref[..., n]) <= tol, (what, n)

import numpy as np
import pytest

from conftest import comp_floors, elementwise_err, max_rel_err
from helpers import DtPolicy, meta_to_params, oracle_comp_run
from oracle import orc
from pyro2_amd import _lib, device

TOL_EXACT = 1e-13
TOL_FAST = 1e-10

# kernel sets under test: 0 staged, 1 fused 2-d tile kernel, 2 fused row-marching
# kernel (autonomous wavefronts) with the library's strip length; 3 = 2 with 11-row
# strips (several strips and ragged last strips on the small test grids)
KSETS = [0, 1, 2, 3]
FUSED_KSETS = [1, 2, 3]


def kset_kw(kset):
    """test id -> parameters: 3 = kernel_set 2 with short strips, 4 = the same with the step
    kernel as the only launch of a step of pyrohip_comp_evolve"""
    if kset == 4:
        return dict(kernel_set=2, march_rows=11, step_launches=1)
    return dict(kernel_set=2, march_rows=11) if kset == 3 else dict(kernel_set=kset)


def dev_params(meta, **kw):
    nx, ny, ng, dx, dy, gamma, lim, flat, z0, z1, delta, cvisc, grav, cfl = meta
    return device.make_comp_params(dx, dy, gamma=gamma, limiter=int(lim),
                                   use_flattening=int(flat), z0=z0, z1=z1,
                                   delta=delta, cvisc=cvisc, grav=grav, **kw), cfl


def comp_state(dev, nx, ny, bcs, ng=4):
    vb = orc.comp_var_bcs(bcs)
    return device.DeviceState(dev, nx, ny, ng, [list(r) for r in vb])


def R(a, ng, lo, hi=None):
    """valid region grown by (lo, hi)"""
    hi = lo if hi is None else hi
    return a[ng - lo:a.shape[0] - ng + hi, ng - lo:a.shape[1] - ng + hi]


@pytest.mark.parametrize("k", range(8))
def test_comp_stages_vs_reference(dev, golden, k):
    """one step from a reference state; every device stage array is compared
    with the array dumped from the reference's own functions on the cells /
    faces inside the interior's domain of dependence"""
    g = golden("comp_stages")
    bcs = [str(b) for b in g[f"c{k}_bc"]]
    meta = g[f"c{k}_meta"]
    P, cfl = dev_params(meta)
    nx, ny, ng = int(meta[0]), int(meta[1]), int(meta[2])
    s = comp_state(dev, nx, ny, bcs)
    U0 = g[f"c{k}_U0"]
    s.upload(U0)
    tol = 0.0 if dev.kind == "emu" else TOL_EXACT
    dt_raw = s.comp_dt(P, cfl)
    assert abs(dt_raw - float(g[f"c{k}_dt_method"])) <= tol * dt_raw
    s.comp_step(P, float(g[f"c{k}_dt"]))

    def chk(name, dev_arr, ref_arr):
        e = max_rel_err(dev_arr, ref_arr)
        assert e <= tol, (k, name, e)

    chk("q", s.comp_stage("q"), g[f"c{k}_q"])
    chk("xi", R(s.comp_stage("xi"), ng, 1), R(g[f"c{k}_xi"], ng, 1))
    # cell-indexed face states: XM[i,j] = U_xr[i,j]; XP[i,j] = U_xl[i+1,j], compared on
    # the cells whose state feeds a needed face: x faces i in [ilo, ihi+1] take
    # XP of cells [ilo-1, ihi] and XM of cells [ilo, ihi+1] (same in y)
    J1 = slice(ng - 1, ng + ny + 1)
    I1 = slice(ng - 1, ng + nx + 1)
    chk("XM", s.comp_stage("XM")[ng:ng + nx + 1, J1], g[f"c{k}_Uxr0"][ng:ng + nx + 1, J1])
    chk("XP", s.comp_stage("XP")[ng - 1:ng + nx, J1], g[f"c{k}_Uxl0"][ng:ng + nx + 1, J1])
    chk("YM", s.comp_stage("YM")[I1, ng:ng + ny + 1], g[f"c{k}_Uyr0"][I1, ng:ng + ny + 1])
    chk("YP", s.comp_stage("YP")[I1, ng - 1:ng + ny], g[f"c{k}_Uyl0"][I1, ng:ng + ny + 1])
    # transverse fluxes: x faces i in [ilo, ihi+1], j in [jlo-1, jhi+1]
    chk("FxT", s.comp_stage("FxT")[ng:ng + nx + 1, ng - 1:ng + ny + 1],
        g[f"c{k}_FxT"][ng:ng + nx + 1, ng - 1:ng + ny + 1])
    chk("FyT", s.comp_stage("FyT")[ng - 1:ng + nx + 1, ng:ng + ny + 1],
        g[f"c{k}_FyT"][ng - 1:ng + nx + 1, ng:ng + ny + 1])
    # final fluxes incl. artificial viscosity on the faces of interior cells
    chk("Fx", s.comp_stage("Fx")[ng:ng + nx + 1, ng:ng + ny],
        g[f"c{k}_Fx"][ng:ng + nx + 1, ng:ng + ny])
    chk("Fy", s.comp_stage("Fy")[ng:ng + nx, ng:ng + ny + 1],
        g[f"c{k}_Fy"][ng:ng + nx, ng:ng + ny + 1])
    U1 = s.download()
    chk("U1", R(U1, ng, 0), R(g[f"c{k}_U1"], ng, 0))
    # ghost cells untouched by the step (in-place semantics of the reference)
    m = np.ones(U1.shape[:2], bool)
    m[ng:-ng, ng:-ng] = False
    assert np.array_equal(U1[m], g[f"c{k}_U1"][m])


@pytest.mark.parametrize("kset", FUSED_KSETS)
@pytest.mark.parametrize("k", range(8))
def test_comp_fused_vs_reference(dev, golden, k, kset):
    """kernel_set 1 / 2 (single fused kernel per step): one step from a reference
    state, end state against the reference's own evolve(); then the cached
    CFL minimum against the oracle's next time step"""
    g = golden("comp_stages")
    bcs = [str(b) for b in g[f"c{k}_bc"]]
    meta = g[f"c{k}_meta"]
    P, cfl = dev_params(meta, **kset_kw(kset))
    nx, ny, ng = int(meta[0]), int(meta[1]), int(meta[2])
    s = comp_state(dev, nx, ny, bcs)
    s.upload(g[f"c{k}_U0"])
    tol = 0.0 if dev.kind == "emu" else TOL_EXACT
    s.comp_step(P, float(g[f"c{k}_dt"]))
    U1 = s.download()
    ref = g[f"c{k}_U1"]
    assert max_rel_err(R(U1, ng, 0), R(ref, ng, 0)) <= tol, k
    m = np.ones(U1.shape[:2], bool)
    m[ng:-ng, ng:-ng] = False
    assert np.array_equal(U1[m], ref[m])
    # next dt: cached interior minimum == full-array minimum after a fill
    Uo = ref.copy()
    orc.comp_fill_bc(Uo, nx, ny, ng, bcs)
    dto = orc.comp_dt(Uo, nx, ny, ng, meta[3], meta[4], meta[5], cfl)
    s.fill_bc()
    assert abs(s.comp_dt(P, cfl) - dto) <= tol * dto


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("k", range(8))
def test_comp_fused_ghost_fill(dev, golden, k, fast):
    """pyrohip_comp_params.fuse_fill: the step takes a state whose ghost cells are NOT
    filled (here: overwritten with NaN) and applies the boundary rules itself -- inside
    the tile kernel where it can (outflow / reflect / periodic sides, no sources), by the
    ordinary fill first elsewhere.  Five steps: bit-identical, ghost frame included, to
    fill_bc() + comp_step() on the eight reference states of comp_stages.npz (all
    boundary combinations, gravity in some)"""
    g = golden("comp_stages")
    bcs = [str(b) for b in g[f"c{k}_bc"]]
    meta = g[f"c{k}_meta"]
    nx, ny, ng = int(meta[0]), int(meta[1]), int(meta[2])
    P, cfl = dev_params(meta, fast_math=fast, kernel_set=1)
    Pf, _ = dev_params(meta, fast_math=fast, kernel_set=1, fuse_fill=1)
    a, b = comp_state(dev, nx, ny, bcs), comp_state(dev, nx, ny, bcs)
    U0 = g[f"c{k}_U0"]
    a.upload(U0)
    a.fill_bc()
    junk = U0.copy()
    m = np.ones(U0.shape[:2], bool)
    m[ng:-ng, ng:-ng] = False
    junk[m] = np.nan
    b.upload(junk)
    dt = float(g[f"c{k}_dt"])
    for step in range(5):
        a.fill_bc()
        a.comp_step(P, dt)
        assert b.comp_dt_is_cached() == (step > 0)
        b.comp_step(Pf, dt)
        A, B = a.download(), b.download()
        assert np.array_equal(A, B), (k, step, np.argwhere(A != B)[:5])
        dt = 0.5 * cfl * min(a.comp_dt(P, 1.0), 1e30)
        assert b.comp_dt(Pf, 1.0) == a.comp_dt(P, 1.0)


def device_comp_run(dev, ic, meta, bcs, tmax, max_steps, ambient=None, **kw):
    """Pyro.run_sim loop (pyro_sim.py:219-256) with the device kernels"""
    P, cfl = dev_params(meta, **kw)
    nx, ny = int(meta[0]), int(meta[1])
    s = comp_state(dev, nx, ny, bcs)
    if any(b in ("hse", "ambient") for b in bcs):
        s.set_user_bc(meta[5], meta[12], meta[4], ambient)
    s.upload(np.nan_to_num(ic))
    pol = DtPolicy(tmax)
    dts = []
    while not (pol.t >= tmax or pol.n >= max_steps):
        s.fill_bc()
        dt = pol(s.comp_dt(P, cfl))
        s.comp_step(P, dt)
        pol.advance(dt)
        dts.append(dt)
    return s.download(), np.array(dts), pol.t


@pytest.mark.parametrize("kset", KSETS)
def test_comp_sedov_64(dev, golden, kset):
    """sedov 64^2 (SURVEY 8(c) fingerprint): 20 steps on the GPU, 6 on emu"""
    g = golden("comp_sedov_64_020")
    bcs = [str(b) for b in g["bc"]]
    nsteps = 20 if dev.kind == "hip" else 6
    U, dts, t = device_comp_run(dev, g["ic"], g["meta"], bcs, 0.1, nsteps, **kset_kw(kset))
    tol = 0.0 if dev.kind == "emu" else TOL_EXACT * nsteps
    assert max_rel_err(dts, g["dts"][:nsteps]) <= tol
    if nsteps == 20:
        assert max_rel_err(U[4:-4, 4:-4], g["final"][4:-4, 4:-4]) <= 1e-12
    else:
        from helpers import oracle_comp_run
        Uo, _, _ = oracle_comp_run(g["ic"], g["meta"], bcs, 0.1, nsteps)
        assert max_rel_err(U[4:-4, 4:-4], Uo[4:-4, 4:-4]) <= tol


@pytest.mark.parametrize("kset", KSETS)
def test_comp_positivity_error(dev, golden, kset):
    """negative internal energy -> PYROHIP_ERR_STATE, like the reference's
    assert (compressible/simulation.py:68-71)"""
    from pyro2_amd._lib import ERR_STATE, PyroHipError
    g = golden("comp_sedov_64_020")
    U = g["ic"].copy()
    U[30, 30, 1] = -1.0
    P, cfl = dev_params(g["meta"], **kset_kw(kset))
    s = comp_state(dev, 64, 64, [str(b) for b in g["bc"]])
    s.upload(U)
    with pytest.raises(PyroHipError) as ei:
        s.comp_step(P, 1e-6)
    assert ei.value.code == ERR_STATE


@pytest.mark.gpu
@pytest.mark.parametrize("kset", KSETS)
def test_comp_reference_regression_sod_x(hip, golden, kset):
    """pyro/test.py:101 -- sod_x_0076.h5 (128x10, limiter 1, reflect y)"""
    g = golden("comp_sod_x_0076")
    bcs = [str(b) for b in g["bc"]]
    U, dts, t = device_comp_run(hip, g["ic"], g["meta"], bcs, float(g["tmax"]), 200,
                                **kset_kw(kset))
    assert len(dts) == 76
    for n in range(3):
        assert max_rel_err(U[4:-4, 4:-4, n], g["gold"][..., n]) < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("kset", KSETS)
@pytest.mark.parametrize("fast", [0, 1])
def test_comp_reference_regression_quad(hip, golden, fast, kset):
    """pyro/test.py:100 -- quad_unsplit_0606.h5 (256^2, 606 steps)"""
    g = golden("comp_quad_0606")
    bcs = [str(b) for b in g["bc"]]
    U, dts, t = device_comp_run(hip, g["ic"], g["meta"], bcs, float(g["tmax"]), 1000,
                                fast_math=fast, **kset_kw(kset))
    assert len(dts) == 606
    for n in range(4):
        e = max_rel_err(U[4:-4, 4:-4, n], g["gold"][..., n])
        assert e < (1e-11 if not fast else TOL_FAST), (n, e)
        if fast:    # element-wise, floor = the variable's median magnitude (measured: 5e-13)
            ref = g["gold"][..., n]
            fl = float(np.median(np.abs(ref))) or float(np.abs(ref).max())
            assert elementwise_err(U[4:-4, 4:-4, n], ref, fl) <= TOL_FAST, n


@pytest.mark.gpu
@pytest.mark.parametrize("kset", KSETS)
@pytest.mark.parametrize("fast", [0, 1])
def test_comp_reference_regression_rt(hip, golden, fast, kset):
    """pyro/test.py:102 -- rt_0945.h5 (64x192, 945 steps, gravity, hse
    boundaries, periodic in x); momenta relative to the largest momentum"""
    g = golden("comp_rt_0945")
    bcs = [str(b) for b in g["bc"]]
    U, dts, t = device_comp_run(hip, g["ic"], g["meta"], bcs, float(g["tmax"]), 10000,
                                fast_math=fast, **kset_kw(kset))
    assert len(dts) == 945
    scale = np.abs(g["gold"]).max(axis=(0, 1))
    err = np.abs(U[4:-4, 4:-4] - g["gold"]).max(axis=(0, 1)) / scale
    assert err.max() < (1e-11 if not fast else TOL_FAST), err
    if fast:    # element-wise after 945 steps of an unstable flow (measured: 2.3e-11)
        for n in range(4):
            ref = g["gold"][..., n]
            fl = float(np.median(np.abs(ref))) or float(np.abs(ref).max())
            assert elementwise_err(U[4:-4, 4:-4, n], ref, fl) <= TOL_FAST, n


@pytest.mark.parametrize("nb", [False, True])
@pytest.mark.parametrize("nx", [34, 35, 36, 47])
def test_comp_wave_short_last_strip(dev, nx, nb):
    """row-marching kernel, 11-row strips on grids with nx % 11 in {1, 2, 3} (and 3 again at
    4 strips): a last strip shorter than the ghost width joins its predecessor, so that the
    boundary strips of a slab always hold the ng rows the neighbour receives (the overlapped
    exchange posts them before the interior strips run).  nb: with neighbours named, i.e.
    the boundary-strips-first launch order.  Sedov-like blast off-centre, 5 steps, against
    the oracle."""
    from sedov_ic import sedov_ic
    ic, meta, bcs = sedov_ic(nx, 40, r_init=0.12)
    Uo, dto, _ = oracle_comp_run(ic, meta, bcs, 0.1, 5)
    P, cfl = dev_params(meta, kernel_set=2, march_rows=11)
    s = comp_state(dev, nx, 40, bcs)
    if nb:
        s.set_neighbours(0, 0)          # launch order only: no communicator in this test
    s.upload(ic)
    pol = DtPolicy(0.1)
    for _ in range(5):
        s.fill_bc()
        dt = pol(s.comp_dt(P, cfl))
        s.comp_step(P, dt)
        pol.advance(dt)
    U = s.download()
    tol = 0.0 if dev.kind == "emu" else 1e-13
    assert max_rel_err(U[4:-4, 4:-4], Uo[4:-4, 4:-4]) <= tol


@pytest.mark.parametrize("kset", [1, 3, 4])
def test_comp_evolve_on_device(dev, golden, kset):
    """pyrohip_comp_evolve: the run_sim loop (ghost fill, the driver's dt policy,
    evolve) enqueued on the device without a host round trip per step, against the
    same steps taken one by one through pyrohip_comp_dt / pyrohip_comp_step --
    dt sequence, time, step count and state bit for bit; in chunks (policy state
    carried from call to call); landing on tmax with steps to spare (the spare
    ones do nothing); and an invalid state in the middle of a call: error, the
    state left behind is the one before the failing step."""
    from helpers import DtPolicy
    from pyro2_amd._lib import ERR_STATE, PyroHipError
    g = golden("comp_sedov_64_020")
    bcs = [str(b) for b in g["bc"]]
    meta = g["meta"]
    P, cfl = dev_params(meta, **kset_kw(kset))
    ic = np.nan_to_num(g["ic"])
    nsteps = 9
    Uref, dref, tref = device_comp_run(dev, ic, meta, bcs, 0.1, nsteps, **kset_kw(kset))
    # one call, and chunks of 4 + 4 + 1
    for chunks in ((nsteps,), (4, 4, 1)):
        s = comp_state(dev, 64, 64, bcs)
        s.upload(ic)
        pol, dts = DtPolicy(0.1), []
        for c in chunks:
            dts += list(s.comp_evolve(P, cfl, pol, c))
        assert dts == list(dref), chunks
        assert pol.n == nsteps and pol.t == tref
        assert np.array_equal(s.download()[4:-4, 4:-4], Uref[4:-4, 4:-4]), chunks
        # the cached CFL minimum of the last step serves the next host-side dt
        s.fill_bc()
        assert s.comp_dt(P, cfl) == pytest.approx(s.comp_dt(P, cfl))
    # tmax inside the call: 9 steps asked, the run ends after fewer
    tmax = float(np.sum(dref[:5])) + 0.3 * float(dref[5])
    Ut, dt_t, t_t = device_comp_run(dev, ic, meta, bcs, tmax, 100, **kset_kw(kset))
    s = comp_state(dev, 64, 64, bcs)
    s.upload(ic)
    pol = DtPolicy(tmax)
    dts = s.comp_evolve(P, cfl, pol, nsteps)
    assert list(dts) == list(dt_t) and len(dts) == 6 and pol.t == tmax == t_t
    assert np.array_equal(s.download()[4:-4, 4:-4], Ut[4:-4, 4:-4])
    # an invalid state after 3 steps
    s = comp_state(dev, 64, 64, bcs)
    s.upload(ic)
    pol = DtPolicy(0.1)
    s.comp_evolve(P, cfl, pol, 3)
    U3 = s.download()
    bad = U3.copy()
    bad[30, 30, 1] = -1.0
    s.upload(bad)
    pol2 = DtPolicy(0.1)
    pol2.t, pol2.n, pol2.dt_old = pol.t, pol.n, pol.dt_old
    with pytest.raises(PyroHipError) as ei:
        s.comp_evolve(P, cfl, pol2, 4)
    assert ei.value.code == ERR_STATE
    assert pol2.n == pol.n and pol2.t == pol.t
    assert np.array_equal(s.download()[4:-4, 4:-4], bad[4:-4, 4:-4])


@pytest.mark.parametrize("kset", [1, 3])
def test_comp_evolve_global_minimum_every_step(dev, golden, kset):
    """decomposed run, device-side stepping: EVERY dt -- the first one of a call included, whose
    CFL minimum comes from a kernel of its own -- is derived from the minimum over all ranks.
    (Round 4, four RCCL ranks on hardware: the first minimum of a pyrohip_comp_evolve call was
    rank-local, the slabs far from the blast ran ahead in time; two ranks hid it by symmetry.)
    The emulated backend has no communicator; its all-reduce folds in a value the test sets as
    \"the other ranks' minimum\" (tests/emu/comm_emu.cpp)."""
    import ctypes
    from helpers import DtPolicy
    from pyro2_amd import _lib
    if dev.kind != "emu":
        pytest.skip("needs the emulated backend's test hook")
    g = golden("comp_sedov_64_020")
    bcs = [str(b) for b in g["bc"]]
    meta = g["meta"]
    P, cfl = dev_params(meta, **kset_kw(kset))
    ic = np.nan_to_num(g["ic"])
    hook = _lib.lib().pyrohip_emu_set_peer_min
    hook.argtypes, hook.restype = [ctypes.c_double], ctypes.c_int
    peer = 1.0e-5                      # far below this state's own minimum
    try:
        hook(peer)
        dev.comm_set_global_dt(True)
        s = comp_state(dev, 64, 64, bcs)
        s.upload(ic)
        pol, dts = DtPolicy(0.1), []
        for n in (4, 3):               # two calls: two "first steps"
            dts += list(s.comp_evolve(P, cfl, pol, n))
    finally:
        dev.comm_set_global_dt(False)
        hook(-1.0)
    ref = DtPolicy(0.1)
    want = []
    for _ in range(7):
        dt = ref(cfl * peer)
        ref.advance(dt)
        want.append(dt)
    assert dts == want
    assert pol.t == ref.t and pol.n == 7


@pytest.mark.parametrize("launches", [1, 3])
@pytest.mark.parametrize("bcs", [("outflow", "outflow", "outflow", "outflow"),
                                 ("reflect", "outflow", "periodic", "periodic"),
                                 ("periodic", "periodic", "reflect", "reflect"),
                                 ("outflow", "reflect", "reflect", "outflow")])
def test_comp_evolve_wave_fill_and_frame(dev, golden, bcs, launches):
    """device-side stepping with the row-marching kernel.  launches = 3: one launch fills the
    ghost cells of the state AND writes the other buffer's ghost frame (evolve.hip:
    k_fill_frame2; corners through the x rule and then the y rule), the policy kernel takes the
    minimum of the wavefronts' CFL partials itself (the default).  launches = 1: the step kernel
    is the ONLY launch of a step -- it reads ghost cells through the boundary rules (index maps,
    odd reflections' signs) instead of a filled frame, its wavefronts fold their CFL minima
    into 64 slots by atomic minimum and every wavefront of the next launch runs the driver's dt
    policy on them (k_ctu_wave<.., ONE>); the final state's ghost cells are filled once at the
    end from the state before its last step.  Both against the same steps taken one by one (two fill
    launches, frame copy, reduction launches): dt sequence and the WHOLE array, ghost frame
    and corners included, bit for bit"""
    from helpers import DtPolicy
    g = golden("comp_sedov_64_020")
    meta = g["meta"]
    ic = np.nan_to_num(g["ic"]).copy()
    rng = np.random.default_rng(3)
    ic[:, :, 2] += 1.e-3 * rng.standard_normal(ic.shape[:2])     # momenta: the odd reflections matter
    ic[:, :, 3] += 1.e-3 * rng.standard_normal(ic.shape[:2])
    nsteps = 7
    kw = dict(kernel_set=2, march_rows=13)
    Uref, dref, tref = device_comp_run(dev, ic, meta, list(bcs), 0.1, nsteps, **kw)
    P, cfl = dev_params(meta, step_launches=launches, **kw)
    for chunks in ((nsteps,), (3, 4), (1, 1, 5)):
        s = comp_state(dev, 64, 64, list(bcs))
        s.upload(ic)
        pol, dts = DtPolicy(0.1), []
        for c in chunks:
            dts += list(s.comp_evolve(P, cfl, pol, c))
        assert dts == list(dref), chunks
        assert np.array_equal(s.download(), Uref), chunks


@pytest.mark.parametrize("launches", [1, 3])
@pytest.mark.parametrize("cut", [2, 3])
def test_comp_evolve_wave_tmax_inside_a_call(dev, golden, launches, cut):
    """tmax ends the run INSIDE a call of the row-marching loop: the iterations behind the last
    step that advanced are inactive (an even and an odd number of them: cut 3 and 2), and what
    they leave -- buffer parity, the ghost frame of the final state -- must be what single steps
    to the same tmax leave: dt sequence, pol.t and the WHOLE array, ghost frame and corners
    included, bit for bit"""
    from helpers import DtPolicy
    g = golden("comp_sedov_64_020")
    meta = g["meta"]
    ic = np.nan_to_num(g["ic"]).copy()
    rng = np.random.default_rng(3)
    ic[:, :, 2] += 1.e-3 * rng.standard_normal(ic.shape[:2])
    ic[:, :, 3] += 1.e-3 * rng.standard_normal(ic.shape[:2])
    bcs = ["reflect", "outflow", "periodic", "periodic"]
    kw = dict(kernel_set=2, march_rows=13)
    _, dref, _ = device_comp_run(dev, ic, meta, bcs, 0.1, 7, **kw)
    tmax = float(np.sum(dref[:cut])) + 0.3 * float(dref[cut])
    Uref, dt_ref, t_ref = device_comp_run(dev, ic, meta, bcs, tmax, 100, **kw)
    P, cfl = dev_params(meta, step_launches=launches, **kw)
    s = comp_state(dev, 64, 64, bcs)
    s.upload(ic)
    pol = DtPolicy(tmax)
    dts = list(s.comp_evolve(P, cfl, pol, 2)) + list(s.comp_evolve(P, cfl, pol, 5))
    assert dts == list(dt_ref)
    assert pol.t == tmax == t_ref
    assert np.array_equal(s.download(), Uref)


@pytest.mark.parametrize("kset", [0, 1, 2])
def test_comp_fast_algebra_supersonic(dev, kset):
    """the fast build's OWN ALGEBRA (hydro.h: characteristic tracing with the projections
    written out and the acoustic terms evaluated lazily; HLLC with a_k = rho_k (S_k - u_k),
    the collapsed star-region flux and the outer-state fluxes) against the bit-faithful build
    on a flow that takes every branch: a Mach-3 stream in +x / -y over half of the domain
    (supersonic faces of both signs in both directions), a counter-stream, a blast and a
    smooth density field (velocities vary smoothly inside each stream: with an exactly uniform
    velocity the flattening switch u(-1) - u(+1) > 0 would hang on the rounding noise of
    momentum / density); reflecting walls in y put -0.0 momenta into the ghost cells (the
    sign BIT picks the upwind side, like np.copysign).  On the emulator both builds divide
    exactly, so the difference is the re-association alone: element-wise 1e-12 after 6
    steps; on the GPU the fast-build tolerance."""
    from sedov_ic import sedov_ic
    nx, ny = 48, 40
    ic, meta, _ = sedov_ic(nx, ny, r_init=0.1)
    bcs = ["outflow", "outflow", "reflect", "reflect"]
    ic = np.nan_to_num(ic)
    x = (np.arange(nx + 8) - 3.5)[:, None] / nx
    y = (np.arange(ny + 8) - 3.5)[None, :] / ny
    rho = 1.0 + 0.4 * np.sin(5 * x + 1) * np.cos(7 * y)
    p = 1.0e-2 * (1.0 + 0.5 * np.cos(3 * x) * np.sin(4 * y))
    p += 2.0 * np.exp(-((x - 0.5) ** 2 + (y - 0.45) ** 2) * 400.0)
    c = np.sqrt(1.4 * p / rho)
    u = np.where(y < 0.5, 3.0, -2.5) * c.mean() * (1.0 + 0.2 * np.sin(9 * x + 2 * y))
    v = np.where(x < 0.5, -3.0, 2.0) * c.mean() * (1.0 + 0.2 * np.cos(4 * x - 7 * y))
    v[:, :6] = 0.0          # at rest next to the lower wall: exact zeros, -0.0 in its ghosts
    ic[..., 0] = rho
    ic[..., 2] = rho * u
    ic[..., 3] = rho * v
    ic[..., 1] = p / 0.4 + 0.5 * rho * (u * u + v * v)
    nsteps = 6
    Ue, dte, _ = device_comp_run(dev, ic, meta, bcs, 1.0, nsteps, fast_math=0, **kset_kw(kset))
    Uf, dtf, _ = device_comp_run(dev, ic, meta, bcs, 1.0, nsteps, fast_math=1, **kset_kw(kset))
    tol = 1e-12 if dev.kind == "emu" else TOL_FAST
    assert max_rel_err(dtf, dte) <= tol
    fl = comp_floors(Ue[4:-4, 4:-4])
    for n in range(4):
        assert elementwise_err(Uf[4:-4, 4:-4, n], Ue[4:-4, 4:-4, n], fl[n]) <= tol, n


def test_comp_fast_path_logic(dev, golden, kset=2):
    """the fast build of the single-launch kernels takes code paths of its own
    (e.g. the transverse Riemann problems use the traced primitive states
    instead of recovering them from the conserved ones).  On the emulator the
    fast build has true divisions and no FMA contraction (the intrinsics are
    GPU-only), so those paths must reproduce the bit-faithful build to rounding:
    a mix-up of states or frames would show at O(1).  On the GPU the same
    comparison holds to the fast-build tolerance."""
    g = golden("comp_sedov_64_020")
    bcs = [str(b) for b in g["bc"]]
    nsteps = 8
    Ue, dte, _ = device_comp_run(dev, g["ic"], g["meta"], bcs, 0.1, nsteps, kernel_set=kset,
                                 fast_math=0)
    Uf, dtf, _ = device_comp_run(dev, g["ic"], g["meta"], bcs, 0.1, nsteps, kernel_set=kset,
                                 fast_math=1, march_rows=13)
    tol = 1e-13 * nsteps if dev.kind == "emu" else TOL_FAST
    assert max_rel_err(dtf, dte) <= tol
    for n in range(4):
        assert max_rel_err(Uf[4:-4, 4:-4, n], Ue[4:-4, 4:-4, n]) <= tol, n


@pytest.mark.parametrize("rows", [0, 7])
def test_comp_march_wide_grid(dev, rows, kset=2):
    """kernel_set 2 on a grid wider than one column strip (56 columns per
    wavefront): 20 x 530 cells = 10 column strips, the last one ragged, short
    strips; an off-centre blast so that no symmetry hides a mix-up of columns.
    Against the staged kernels (validated stage by stage above): bit-identical
    in the bit-faithful build"""
    from sedov_ic import sedov_ic
    nx, ny = 20, 530
    ic, meta, bcs = sedov_ic(nx, ny, r_init=0.02, xmin=0.0, xmax=0.2, ymin=0.0, ymax=5.3)
    # move the energy peak off the centre, add a smooth density / velocity field
    ic = np.nan_to_num(ic)
    x = (np.arange(nx + 8) - 3.5)[:, None] / nx
    y = (np.arange(ny + 8) - 3.5)[None, :] / ny
    ic[..., 0] = 1.0 + 0.3 * np.sin(7 * x + 3) * np.cos(23 * y)
    ic[..., 2] = 0.1 * ic[..., 0] * np.cos(11 * y + x)
    ic[..., 3] = -0.2 * ic[..., 0] * np.sin(5 * x) * np.sin(17 * y)
    ic[..., 1] += 0.5 * (ic[..., 2] ** 2 + ic[..., 3] ** 2) / ic[..., 0]
    ic[..., 1] += 0.4 * np.exp(-((x - 0.3) ** 2 + (y - 0.47) ** 2) * 4000.0)
    ic[..., 1] += 0.7 * np.exp(-((x - 0.8) ** 2 + (y - 0.935) ** 2) * 4000.0)
    nsteps = 3
    Us, dts_s, _ = device_comp_run(dev, ic, meta, bcs, 10.0, nsteps, kernel_set=0)
    Um, dts_m, _ = device_comp_run(dev, ic, meta, bcs, 10.0, nsteps, kernel_set=kset,
                                   march_rows=rows)
    tol = 0.0 if dev.kind == "emu" else TOL_EXACT * nsteps
    assert max_rel_err(dts_m, dts_s) <= tol
    for n in range(4):
        assert max_rel_err(Um[..., n], Us[..., n]) <= tol, n


@pytest.mark.gpu
@pytest.mark.parametrize("kset", KSETS)
@pytest.mark.parametrize("fast", [0, 1])
def test_comp_sedov_512_vs_oracle(hip, fast, kset):
    """sedov at 512^2 (inputs.sedov physics), 30 steps, against the oracle on
    identical inputs; 1e-10 is the north_star tolerance"""
    from sedov_ic import sedov_ic
    nx = 512
    ic, meta, bcs = sedov_ic(nx)
    from helpers import oracle_comp_run
    Uo, dto, _ = oracle_comp_run(ic, meta, bcs, 0.1, 30)
    U, dts, _ = device_comp_run(hip, ic, meta, bcs, 0.1, 30, fast_math=fast, **kset_kw(kset))
    tol = TOL_FAST if fast else 1e-12
    assert max_rel_err(dts, dto) <= tol
    assert_state_close(U[4:-4, 4:-4], Uo[4:-4, 4:-4], tol, fast, "sedov 512")
    # conservation of mass and energy away from the (outflow) boundary
    assert abs(U[4:-4, 4:-4, 0].sum() - ic[4:-4, 4:-4, 0].sum()) < 1e-9 * nx * nx


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [0, 1])
def test_comp_sedov_8192_vs_oracle_window(hip, golden, fast):
    """north_star's target size (Sedov 8192^2), checked like the 16384^2 case below
    (oracle/gen_fullsize.py --window8192)"""
    _sedov_window_check(hip, golden("comp_sedov_8192_window"), 8192, fast)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [0, 1])
def test_comp_sedov_16384_vs_oracle_window(hip, golden, fast):
    _sedov_window_check(hip, golden("comp_sedov_16384_window"), 16384, fast)


def _sedov_window_check(hip, g, nx, fast):
    """the bench's own workload and size (Sedov 16384^2, 25 steps from t = 0,
    default kernel set) against the C oracle.  The oracle ran the central
    1024^2 window with the full grid's cell coordinates (oracle/gen_fullsize.py
    --window16384): the disturbance (half-width 177 cells after 25 steps) never
    reaches the window's edge, so window == full grid there, and every cell
    outside must still hold the ambient state bit for bit.  dt sequence, a 64x64
    lattice, row / column sums of the window and a dense 16x256 patch across the
    shock; fast build element-wise (1e-10), bit-faithful build 1e-12."""
    from pyro2_amd.compressible.problems.sedov import sedov_state
    ng, nsteps = 4, int(g["nsteps"])
    lo, W = int(g["lo"]), int(g["width"])
    s = comp_state(hip, nx, nx, ["outflow"] * 4)
    for r0 in range(0, nx + 2 * ng, 512):
        nr = min(512, nx + 2 * ng - r0)
        s.upload_rows(r0, sedov_state(nx, nx, ng, 0.0, 1.0, 0.0, 1.0, 1.4, 0.01, 4, i0=r0, ni=nr))
    P = device.make_comp_params(1.0 / nx, 1.0 / nx, fast_math=fast, kernel_set=-1)
    pol = DtPolicy(0.1)
    dts = []
    for _ in range(nsteps):
        s.fill_bc()
        dt = pol(s.comp_dt(P, 0.8))
        s.comp_step(P, dt)
        pol.advance(dt)
        dts.append(dt)
    tol = TOL_FAST if fast else 1e-12
    assert max_rel_err(np.array(dts), g["dts"]) <= tol
    I = s.download_rows(ng + lo, W)[:, ng + lo:ng + lo + W]
    step = W // 64
    assert_state_close(I[::step, ::step], g["samples"], tol, fast, "lattice")
    assert_state_close(I[W // 2 - 8:W // 2 + 8, W // 2:W // 2 + 256], g["patch"], tol, fast, "patch")
    umax = g["umax"]
    for n in range(4):
        for ax, key in ((1, "row_sums"), (0, "col_sums")):
            ref = g[key][:, n]
            assert np.abs(I[..., n].sum(axis=ax) - ref).max() <= tol * max(np.abs(ref).max(), W * umax[n] * 1e-3)
    # outside the window: untouched ambient gas (rows next to the window and far away)
    amb = sedov_state(nx, nx, ng, 0.0, 1.0, 0.0, 1.0, 1.4, 0.01, 4, i0=0, ni=1)[0, 0]
    for r in (ng, ng + lo - 1, ng + lo + W, ng + nx - 1):
        row = s.download_rows(r, 1)[0, ng:-ng]
        assert np.array_equal(row, np.broadcast_to(amb, row.shape)), r
    assert np.array_equal(I[:, 0], np.broadcast_to(amb, I[:, 0].shape))


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [0, 1])
def test_comp_sedov_developed_vs_oracle(hip, golden, fast):
    """the DEVELOPED-flow state the bench's `also.sedov_developed` leg times (a 1024^2
    Sedov blast at t = 0.1, ~2300 steps: 30 % of the cells shocked) against the C oracle
    (oracle/gen_fullsize.py --developed1024): dt sequence, a 64 x 64 lattice, row / column
    sums and a dense patch from the centre across the shock.  Device-side stepping
    (pyrohip_comp_evolve), default kernel set; fast build element-wise 1e-10,
    bit-faithful build 1e-12."""
    from sedov_ic import sedov_ic
    g = golden("comp_sedov_1024_developed")
    nx, ng, nsteps = 1024, 4, int(g["nsteps"])
    ic, meta, bcs = sedov_ic(nx)
    s = comp_state(hip, nx, nx, bcs)
    s.upload(ic)
    P = device.make_comp_params(1.0 / nx, 1.0 / nx, fast_math=fast, kernel_set=-1)
    pol = DtPolicy(0.1)
    dts = []
    while pol.t < 0.1 and pol.n < nsteps + 10:
        dts.extend(s.comp_evolve(P, 0.8, pol, min(256, nsteps + 10 - pol.n)))
    dts = np.array(dts)
    tol = TOL_FAST if fast else 1e-12
    assert len(dts) == nsteps
    assert max_rel_err(dts[:-1], g["dts"][:-1]) <= tol          # the last one is the clip to tmax
    assert abs(dts[-1] - g["dts"][-1]) <= tol * g["dts"][-2]
    I = s.download()[ng:-ng, ng:-ng]
    step = nx // 64
    assert_state_close(I[::step, ::step], g["samples"], tol, fast, "lattice")
    assert_state_close(I[nx // 2 - 8:nx // 2 + 8, nx // 2:], g["patch"], tol, fast, "patch")
    umax = g["umax"]
    for n in range(4):
        for ax, key in ((1, "row_sums"), (0, "col_sums")):
            ref = g[key][:, n]
            assert np.abs(I[..., n].sum(axis=ax) - ref).max() <= tol * max(np.abs(ref).max(), nx * umax[n] * 1e-3)
    assert abs(float((np.abs(I[..., 0] - 1.0) > 1e-8).mean()) - float(g["shocked"])) < 1e-3


@pytest.mark.gpu
def test_comp_sedov_4096_properties(hip):
    """BASELINE config 2 size (sedov 4096^2): the oracle cannot run this in
    test time, so size-independent properties after 12 steps -- (i) the fused
    and the staged kernel sets (independent code paths, bit-faithful build)
    agree to 1e-12, (ii) the default fast build stays within 1e-10 of them,
    (iii) mass and energy are conserved to round-off (the blast is far from the
    outflow boundary), (iv) the solution keeps the x <-> y symmetry of the
    problem, (v) the time steps of all three runs agree"""
    from sedov_ic import sedov_ic
    nx = 4096
    ic, meta, bcs = sedov_ic(nx)
    runs = {}
    for name, kw in (("fused", dict(fast_math=0, kernel_set=1)),
                     ("staged", dict(fast_math=0, kernel_set=0)),
                     ("fast", dict(fast_math=1, kernel_set=1))):
        U, dts, _ = device_comp_run(hip, ic, meta, bcs, 0.1, 12, **kw)
        runs[name] = (U[4:-4, 4:-4].copy(), dts)
        del U
    Uf, df = runs["fused"]
    for other, tol in (("staged", 1e-12), ("fast", TOL_FAST)):
        Uo, do = runs[other]
        assert max_rel_err(do, df) <= tol
        for n in range(4):
            scale = np.abs(Uf[..., n]).max()
            assert np.abs(Uo[..., n] - Uf[..., n]).max() <= tol * max(scale, 1.0), (other, n)
    I0 = ic[4:-4, 4:-4]
    for n in (0, 1):   # density, energy
        assert abs(Uf[..., n].sum() - I0[..., n].sum()) <= 1e-12 * np.abs(I0[..., n]).sum()
    # transpose symmetry: rho, E symmetric; x-momentum(i,j) = y-momentum(j,i)
    assert np.abs(Uf[..., 0] - Uf[..., 0].T).max() <= 1e-10 * np.abs(Uf[..., 0]).max()
    assert np.abs(Uf[..., 2] - Uf[..., 3].T).max() <= 1e-10 * np.abs(Uf[..., 2]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [0, 1])
def test_comp_sedov_4096_vs_oracle_samples(hip, golden, fast):
    """BASELINE config 2 at full size against the C oracle (oracle/
    gen_fullsize.py: sedov 4096^2, 25 steps, ~10 min of CPU): dt sequence, a
    64x64 lattice of the state and its row / column sums per variable"""
    from sedov_ic import sedov_ic
    g = golden("comp_sedov_4096_samples")
    nx, nsteps = 4096, int(g["nsteps"])
    ic, meta, bcs = sedov_ic(nx)
    U, dts, t = device_comp_run(hip, ic, meta, bcs, 0.1, nsteps, fast_math=fast, kernel_set=-1)
    tol = TOL_FAST if fast else 1e-12
    assert max_rel_err(dts, g["dts"]) <= tol
    I = U[4:-4, 4:-4]
    step = nx // 64
    umax = g["umax"]
    assert_state_close(I[::step, ::step], g["samples"], tol, fast, "lattice")
    for n in range(4):
        for ax, key in ((1, "row_sums"), (0, "col_sums")):
            ref = g[key][:, n]
            assert np.abs(I[..., n].sum(axis=ax) - ref).max() <= tol * max(np.abs(ref).max(), nx * umax[n] * 1e-3)


@pytest.mark.parametrize("kset", KSETS)
def test_comp_gravity_run(dev, kset):
    """gravity sources (apply_source_terms + predictor-corrector,
    unsplit_fluxes.py:247-330, simulation.py:406-423): a perturbed stratified
    atmosphere between reflecting walls, periodic in x, against the oracle"""
    from helpers import oracle_comp_run
    nx, ny, ng = 24, 32, 4
    gamma, grav = 1.4, -1.0
    dx, dy = 1.0 / nx, 2.0 / ny
    x = (np.arange(nx + 2 * ng) - ng + 0.5) * dx
    y = (np.arange(ny + 2 * ng) - ng + 0.5) * dy
    X, Y = np.meshgrid(x, y, indexing="ij")
    rho = np.where(Y < 1.0, 1.0, 2.0)
    p = 5.0 + grav * np.where(Y < 1.0, Y, 1.0 + 2.0 * (Y - 1.0))
    v = 0.05 * np.cos(2 * np.pi * X) * np.exp(-((Y - 1.0) / 0.2) ** 2)
    ic = np.zeros((nx + 2 * ng, ny + 2 * ng, 4))
    ic[..., 0] = rho
    ic[..., 3] = rho * v
    ic[..., 1] = p / (gamma - 1.0) + 0.5 * rho * v * v
    meta = np.array([nx, ny, ng, dx, dy, gamma, 2, 1, 0.75, 0.85, 0.33, 0.1, grav, 0.8])
    bcs = ["periodic", "periodic", "reflect", "reflect"]
    nsteps = 8 if dev.kind == "emu" else 40
    Uo, dto, _ = oracle_comp_run(ic, meta, bcs, 10.0, nsteps)
    U, dts, _ = device_comp_run(dev, ic, meta, bcs, 10.0, nsteps, **kset_kw(kset))
    tol = 0.0 if dev.kind == "emu" else 1e-12
    assert max_rel_err(dts, dto) <= tol
    for n in range(4):
        assert max_rel_err(U[4:-4, 4:-4, n], Uo[4:-4, 4:-4, n]) <= tol, n
    assert np.abs(U[4:-4, 4:-4, 3]).max() > 1e-3   # gravity did something


@pytest.mark.parametrize("kset", KSETS)
@pytest.mark.parametrize("k", range(6))
def test_comp_cgf_and_sponge(dev, golden, k, kset):
    """SURVEY 8 row f2 on the device: CGF Riemann solver (incl. the solid-wall
    rule) and the sponge, one step from reference states"""
    g = golden("comp_stages_f2")
    bcs = [str(b) for b in g[f"c{k}_bc"]]
    meta = g[f"c{k}_meta"]
    sp = g[f"c{k}_sponge"]
    solid = [int(b == "reflect") for b in bcs]
    P, cfl = dev_params(meta, **kset_kw(kset), riemann=str(g[f"c{k}_riemann"]),
                        solid_xl=solid[0], solid_yl=solid[2],
                        sponge=tuple(sp[1:]) if sp[0] else None)
    nx, ny, ng = int(meta[0]), int(meta[1]), int(meta[2])
    s = comp_state(dev, nx, ny, bcs)
    s.upload(g[f"c{k}_U0"])
    s.comp_step(P, float(g[f"c{k}_dt"]))
    tol = (1e-15 if sp[0] else 0.0) if dev.kind == "emu" else TOL_EXACT
    if kset == 0:
        for nm, sl in (("FxT", (slice(ng, ng + nx + 1), slice(ng - 1, ng + ny + 1))),
                       ("FyT", (slice(ng - 1, ng + nx + 1), slice(ng, ng + ny + 1))),
                       ("Fx", (slice(ng, ng + nx + 1), slice(ng, ng + ny))),
                       ("Fy", (slice(ng, ng + nx), slice(ng, ng + ny + 1)))):
            assert max_rel_err(s.comp_stage(nm)[sl], g[f"c{k}_{nm}"][sl]) <= (0.0 if dev.kind == "emu" else TOL_EXACT), (k, nm)
    U1 = s.download()
    ref = g[f"c{k}_U1"]
    if sp[0]:   # the sponge also acts on the ghost cells
        assert max_rel_err(U1, ref) <= tol, k
    else:
        assert max_rel_err(R(U1, ng, 0), R(ref, ng, 0)) <= tol, k


@pytest.mark.parametrize("kset", KSETS)
@pytest.mark.parametrize("k", range(4))
def test_comp_hse_ambient_runs(dev, golden, k, kset):
    """gravity with the hse / ambient user boundaries
    (compressible/BC.py) filled on the device, whole runs of the reference
    (rt / hse problems, periodic / outflow / reflecting x sides, HLLC and CGF)"""
    g = golden("comp_hse")
    pre = f"c{k}_"
    meta, bcs = g[pre + "meta"], [str(b) for b in g[pre + "bc"]]
    riemann = "CGF" if k == 1 else "HLLC"
    solid = [int(b == "reflect") for b in bcs]
    P, cfl = dev_params(meta, **kset_kw(kset), riemann=riemann, solid_xl=solid[0],
                        solid_yl=solid[2])
    nx, ny, ng = int(meta[0]), int(meta[1]), int(meta[2])
    s = comp_state(dev, nx, ny, bcs)
    with pytest.raises(_lib.PyroHipError):
        s.fill_bc()                      # parameters of the user boundary missing
    s.set_user_bc(meta[5], meta[12], meta[4], g[pre + "ambient"])
    s.upload(np.nan_to_num(g[pre + "ic"]))   # NaNs only in never-read y ghost rows
    dts_ref = g[pre + "dts"]
    if dev.kind == "emu" and kset == 0 and k != 2:
        pytest.skip("emulated backend: staged set on the smallest case only (time)")
    # from step 8 on the CFL limit takes over, and its minimum sits in the hse
    # ghost rows; the emulated backend runs that far on the smallest case only
    nsteps = len(dts_ref) if dev.kind == "hip" else (9 if (k == 2 and kset == 1) else 4)
    f0, mx = g[pre + "drv"]
    pol = DtPolicy(1.e30, f0, mx)
    dts = []
    for _ in range(nsteps):
        s.fill_bc()
        dt = pol(s.comp_dt(P, cfl))
        s.comp_step(P, dt)
        pol.advance(dt)
        dts.append(dt)
    # the CGF run holds one face where the shim's libm pow differs from x*x
    # by an ulp (tests/test_oracle_golden.py::test_oracle_hse_runs): compare
    # with the oracle's default arithmetic there
    from helpers import oracle_comp_run
    Uo, dto, _ = oracle_comp_run(g[pre + "ic"], meta, bcs, 1.e30, nsteps, f0, mx,
                                 ambient=tuple(g[pre + "ambient"]), riemann=riemann)
    tol = 0.0 if dev.kind == "emu" else TOL_EXACT * nsteps
    assert max_rel_err(np.array(dts), dto) <= tol
    if k != 1:
        assert max_rel_err(np.array(dts), dts_ref[:nsteps]) <= tol
    U = s.download()
    scale = np.maximum(np.abs(Uo[ng:-ng, ng:-ng]).max(axis=(0, 1)), 1e-3)
    err = (np.abs(U - Uo)[ng:-ng, ng:-ng] / scale).max()
    assert err <= tol, err
    # ghost cells: as the last fill left them
    assert np.abs(np.nan_to_num(U) - np.nan_to_num(Uo)).max() <= tol * scale.max()
    # and one more fill against the reference's filled state
    if nsteps == len(dts_ref) and k != 1:
        s.fill_bc()
        assert (np.abs(s.download() - g[pre + "filled"]) / scale).max() <= tol


@pytest.mark.parametrize("k", range(4))
def test_compressible_rk(dev, golden, k):
    """compressible_rk right-hand side and RK2 / TVD2 / TVD3 /
    RK4 runs (HLLC + CGF, gravity + hse, sponge) against the reference"""
    from helpers import RK_TABLEAU, oracle_rk_run
    g = golden("comp_rk")
    pre = f"c{k}_"
    meta, bcs = g[pre + "meta"], [str(b) for b in g[pre + "bc"]]
    method, riemann, sp = str(g[pre + "method"]), str(g[pre + "riemann"]), g[pre + "sponge"]
    solid = [int(b == "reflect") for b in bcs]
    kw = dict(riemann=riemann, solid_xl=solid[0], solid_yl=solid[2],
              sponge=tuple(sp[1:]) if sp[0] else None)
    P, cfl = dev_params(meta, **kw)
    nx, ny, ng = int(meta[0]), int(meta[1]), int(meta[2])
    I = (slice(ng, -ng), slice(ng, -ng))
    a, b = RK_TABLEAU[method]
    ns = len(b)

    def states():
        s = comp_state(dev, nx, ny, bcs)
        y = comp_state(dev, nx, ny, bcs)
        kst = device.DeviceState(dev, nx, ny, ng, [["outflow"] * 4] * (4 * ns))
        for t in (s, y):
            if "hse" in bcs:
                t.set_user_bc(meta[5], meta[12], meta[4], None)
        return s, y, kst
    tol = 0.0 if dev.kind == "emu" else TOL_EXACT
    # right-hand side of a reference state (CGF: against the oracle's default
    # arithmetic, see test_oracle_hse_runs)
    s, y, kst = states()
    s.upload(g[pre + "U0"])
    s.comp_rk_rhs(P, kst, 0)
    kd = kst.download()[:, :, :4]
    kref = g[pre + "k"] if riemann != "CGF" else orc.comp_rk_rhs(
        g[pre + "U0"].copy(), meta_to_params(meta, bcs, **{k_: v for k_, v in kw.items()
                                                            if k_ in ("riemann", "sponge")})[0])[1]
    scale = np.maximum(np.abs(kref[I]).max(axis=(0, 1)), 1e-3)
    assert (np.abs(kd[I] - kref[I]) / scale).max() <= tol * 10
    # runs
    dts_ref = g[pre + "dts"]
    nsteps = len(dts_ref) if dev.kind == "hip" else 2
    f0, mx = g[pre + "drv"]
    s, y, kst = states()
    s.upload(np.nan_to_num(g[pre + "ic"]))
    pol = DtPolicy(1.e30, f0, mx)
    for n in range(nsteps):
        s.fill_bc()
        dt = pol(s.comp_rk_dt(P, cfl))
        assert abs(dt / dts_ref[n] - 1) <= max(tol * nsteps * 10, 1e-13)
        for st in range(ns):
            if st == 0:
                cur = s
            else:
                y.lincomb(s, kst, [dt * a[st][j] for j in range(st)])
                y.fill_bc()
                cur = y
            cur.comp_rk_rhs(P, kst, st)
        s.lincomb(s, kst, [dt * b[st] for st in range(ns)])
        pol.advance(dt)
    over = {"riemann": riemann}
    if sp[0]:
        over["sponge"] = tuple(sp[1:])
    Uo, _ = oracle_rk_run(g[pre + "ic"], meta, bcs, nsteps, method, f0, mx, **over)
    U = s.download()
    scale = np.maximum(np.abs(Uo[I]).max(axis=(0, 1)), 1e-3)
    assert (np.abs(U[I] - Uo[I]) / scale).max() <= tol * nsteps * 10


@pytest.mark.parametrize("kset", [-1, 2])
@pytest.mark.parametrize("k", [0, 1])
def test_pyro_compressible_rk(dev, golden, k, kset, tmp_path, monkeypatch):
    """compressible_rk through Pyro against runs of the reference (dt sequence, end state); kset
    2: every right-hand side by one launch of the row-marching kernel's method-of-lines instance
    (what the library picks from 2048^2 cells on), -1: the staged kernels at these sizes"""
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    from pyro2_amd.pyro_sim import Pyro
    g = golden("comp_rk")
    pre = f"c{k}_"
    prob, d = [("sedov", {"mesh.nx": 16, "mesh.ny": 16, "sedov.r_init": 0.2}),
               ("rt", {"mesh.nx": 12, "mesh.ny": 36, "rt.amp": 0.4,
                       "compressible.temporal_method": "TVD3"})][k]
    d = dict(d, **{"gpu.kernel_set": kset, "gpu.fast_math": 0})
    nsteps = len(g[pre + "dts"]) if dev.kind == "hip" else 2
    p = Pyro("compressible_rk")
    p.initialize_problem(prob, inputs_dict=dict(d, **{"driver.max_steps": nsteps}))
    dts = []
    while not p.sim.finished():
        p.single_step()
        dts.append(p.sim.dt)
    assert max_rel_err(np.array(dts), g[pre + "dts"][:nsteps]) < 1e-12
    if nsteps == len(g[pre + "dts"]):
        U = np.asarray(p.sim.cc_data.data)
        fin = g[pre + "final"]
        scale = np.maximum(np.abs(fin[4:-4, 4:-4]).max(axis=(0, 1)), 1e-3)
        assert (np.abs(U - fin)[4:-4, 4:-4] / scale).max() < 1e-11


@pytest.mark.parametrize("kset", KSETS)
@pytest.mark.parametrize("k", range(4))
def test_comp_hllc_lm(dev, golden, k, kset):
    """low-Mach HLLC (compressible.riemann = HLLC_lm) on the
    device, one step from reference states, against the oracle's default
    arithmetic (x*x, like numba and the kernels) and the reference dumps"""
    g = golden("comp_stages_lm")
    bcs = [str(b) for b in g[f"c{k}_bc"]]
    meta = g[f"c{k}_meta"]
    P, cfl = dev_params(meta, **kset_kw(kset), riemann="HLLC_lm")
    nx, ny, ng = int(meta[0]), int(meta[1]), int(meta[2])
    s = comp_state(dev, nx, ny, bcs)
    if "hse" in bcs:
        s.set_user_bc(meta[5], meta[12], meta[4], None)
    s.upload(g[f"c{k}_U0"])
    s.comp_step(P, float(g[f"c{k}_dt"]))
    Po, _ = meta_to_params(meta, bcs, riemann="HLLC_lm")
    Uo = g[f"c{k}_U0"].copy()
    rc, st = orc.comp_step(Uo, Po, float(g[f"c{k}_dt"]), stages=True)
    tol = 0.0 if dev.kind == "emu" else TOL_EXACT
    if kset == 0:
        for nm, sl in (("FxT", (slice(ng, ng + nx + 1), slice(ng - 1, ng + ny + 1))),
                       ("FyT", (slice(ng - 1, ng + nx + 1), slice(ng, ng + ny + 1))),
                       ("Fx", (slice(ng, ng + nx + 1), slice(ng, ng + ny))),
                       ("Fy", (slice(ng, ng + nx), slice(ng, ng + ny + 1)))):
            assert max_rel_err(s.comp_stage(nm)[sl], st[nm][sl]) <= tol, (k, nm)
    U1 = s.download()
    scale = np.maximum(np.abs(Uo[ng:-ng, ng:-ng]).max(axis=(0, 1)), 1e-3)
    assert (np.abs(U1 - Uo)[ng:-ng, ng:-ng] / scale).max() <= tol
    assert (np.abs(U1 - g[f"c{k}_U1"])[ng:-ng, ng:-ng] / scale).max() <= 1e-13


@pytest.mark.parametrize("kset", KSETS)
def test_comp_ramp_boundary(dev, golden, kset):
    """the time-dependent "ramp" boundary of the double Mach
    reflection problem (compressible/BC.py:178-296) filled on the device; run
    and final ghost fill against the reference"""
    from test_oracle_golden import oracle_ramp_run
    g = golden("comp_ramp")
    meta, bcs, dom = g["meta"], [str(b) for b in g["bc"]], g["domain"]
    P, cfl = dev_params(meta, **kset_kw(kset))
    nx, ny, ng = int(meta[0]), int(meta[1]), int(meta[2])
    s = comp_state(dev, nx, ny, bcs)
    with pytest.raises(_lib.PyroHipError):
        s.fill_bc()
    s.upload(g["ic"])
    nsteps = len(g["dts"]) if dev.kind == "hip" else 4
    f0, mx = g["drv"]
    pol = DtPolicy(1.e30, f0, mx)

    def push(t):
        s.set_ramp_bc(**orc.ramp_params(nx, ny, ng, dom[0], dom[1], dom[2], dom[3], meta[5], t))
    for n in range(nsteps):
        push(pol.t)
        s.fill_bc()
        dt = pol(s.comp_dt(P, cfl))
        assert abs(dt / g["dts"][n] - 1) <= 1e-12
        s.comp_step(P, dt)
        pol.advance(dt)
    Uo, _, t, _, _ = oracle_ramp_run(g, nsteps)
    tol = 0.0 if dev.kind == "emu" else TOL_EXACT * nsteps
    U = s.download()
    scale = np.abs(Uo).max(axis=(0, 1))
    assert (np.abs(U - Uo) / scale).max() <= tol
    if nsteps == len(g["dts"]):
        push(pol.t)
        s.fill_bc()
        assert (np.abs(s.download() - g["filled"]) / scale).max() <= tol


@pytest.mark.parametrize("kset", KSETS)
@pytest.mark.parametrize("k", range(3))
def test_comp_problem_sources(dev, golden, k, kset):
    """the heating source of the heating / plume / convection
    problems on the device (convection: + gravity, sponge, reflecting wall,
    ambient boundary, density floor); one step from a reference state and a
    short run against the reference"""
    from test_oracle_golden import _heat_case
    from helpers import oracle_comp_run
    g = golden("comp_heating")
    pre, bcs, over = _heat_case(g, k)
    meta = g[pre + "meta"]
    nx, ny, ng = int(meta[0]), int(meta[1]), int(meta[2])
    I = (slice(ng, -ng), slice(ng, -ng))
    solid = [int(b == "reflect") for b in bcs]
    P, cfl = dev_params(meta, **kset_kw(kset), solid_xl=solid[0], solid_yl=solid[2],
                        small_dens=over["small_dens"], sponge=over.get("sponge"),
                        heat_rate=over["heating"][0])

    def state():
        s = comp_state(dev, nx, ny, bcs)
        if any(b in ("hse", "ambient") for b in bcs):
            s.set_user_bc(meta[5], meta[12], meta[4], g[pre + "ambient"])
        s.set_heating(g[pre + "prof"])
        return s
    tol = 0.0 if dev.kind == "emu" else TOL_EXACT
    s = state()
    s.upload(g[pre + "U0"])
    s.comp_step(P, float(g[pre + "dt"]))
    ref = g[pre + "U1"]
    scale = np.maximum(np.abs(ref[I]).max(axis=(0, 1)), 1e-3)
    U1 = s.download()
    sel = slice(None) if g[pre + "sponge"][0] else I      # the sponge also acts on ghost cells
    tol1 = max(tol, 1e-15) if g[pre + "sponge"][0] else tol      # cos() in the sponge
    assert (np.abs(U1 - ref)[sel] / scale).max() <= tol1
    if kset == 0:
        for nm, sl in (("Fx", (slice(ng, ng + nx + 1), slice(ng, ng + ny))),
                       ("Fy", (slice(ng, ng + nx), slice(ng, ng + ny + 1)))):
            assert max_rel_err(s.comp_stage(nm)[sl], g[pre + nm][sl]) <= tol, nm
    # run
    nsteps = len(g[pre + "dts"]) if dev.kind == "hip" else 4
    f0, mx = g[pre + "drv"]
    s = state()
    s.upload(np.nan_to_num(g[pre + "ic"]))
    pol = DtPolicy(1.e30, f0, mx)
    for n in range(nsteps):
        s.fill_bc()
        dt = pol(s.comp_dt(P, cfl))
        assert abs(dt / g[pre + "dts"][n] - 1) <= 1e-12
        s.comp_step(P, dt)
        pol.advance(dt)
    Uo, _, _ = oracle_comp_run(g[pre + "ic"], meta, bcs, 1.e30, nsteps, f0, mx,
                               ambient=tuple(g[pre + "ambient"]), **over)
    assert (np.abs(s.download() - Uo)[I] / scale).max() <= max(tol * nsteps, 1e-14 if g[pre + "sponge"][0] else 0.0)


# ---------------------------------------------------------------------------
# SphericalPolar geometry
# ---------------------------------------------------------------------------
SPH_NAMES = ("Lx", "Ly", "Ax", "Ay", "V", "dlogAx", "dlogAy", "x2d", "sint", "sinb", "sinc")


def sph_arrays(g, pre):
    return {n: g[pre + "g_" + n] for n in SPH_NAMES}


@pytest.mark.parametrize("k", range(3))
def test_comp_spherical(dev, golden, k):
    """the compressible solver on a SphericalPolar grid through the C ABI
    (pyrohip_state_set_geometry): one step from a reference state -- stages and
    end state against the oracle (bit-identical in the exact build) and the
    reference's dumps -- and a short run with its time steps"""
    from helpers import DtPolicy
    from test_oracle_golden import sph_geom
    g = golden("comp_spherical")
    pre = f"c{k}_"
    bcs = [str(b) for b in g[pre + "bc"]]
    meta = g[pre + "meta"]
    solid = [int(b in ("reflect", "reflect-even", "reflect-odd", "dirichlet")) for b in bcs]
    P, cfl = dev_params(meta, kernel_set=0, riemann="CGF", solid_xl=solid[0], solid_yl=solid[2])
    nx, ny, ng = int(meta[0]), int(meta[1]), int(meta[2])
    dom = g[pre + "g_domain"]
    s = comp_state(dev, nx, ny, bcs)
    s.set_geometry(sph_arrays(g, pre), dom[0], dom[2])
    s.upload(g[pre + "U0"])
    dt = float(g[pre + "dt"])
    if str(g[pre + "problem"]) != "advect":
        assert abs(s.comp_dt(P, cfl) / dt - 1) < 1e-13
    s.comp_step(P, dt)
    Po, _ = meta_to_params(meta, bcs, riemann="CGF")
    geom = sph_geom(g, pre)
    Uo = g[pre + "U0"].copy()
    rc, st = orc.comp_step(Uo, Po, dt, stages=True, geom=geom)
    assert rc == 0
    tol = 0.0 if dev.kind == "emu" else TOL_EXACT
    for nm, sl in (("FxT", (slice(ng, ng + nx + 1), slice(ng - 1, ng + ny + 1))),
                   ("FyT", (slice(ng - 1, ng + nx + 1), slice(ng, ng + ny + 1))),
                   ("Fx", (slice(ng, ng + nx + 1), slice(ng, ng + ny))),
                   ("Fy", (slice(ng, ng + nx), slice(ng, ng + ny + 1)))):
        assert max_rel_err(s.comp_stage(nm)[sl], st[nm][sl]) <= tol, (k, nm)
    I = (slice(ng, -ng), slice(ng, -ng))
    U1 = s.download()
    scale = np.maximum(np.abs(Uo[I]).max(axis=(0, 1)), 1e-3)
    assert (np.abs(U1 - Uo)[I] / scale).max() <= tol
    assert (np.abs(U1 - g[pre + "U1"])[I] / scale).max() <= 1e-12
    # a run from the initial condition with the driver's dt policy
    f0, mx = g[pre + "drv"]
    fix = 0.005 if str(g[pre + "problem"]) == "advect" else -1.0
    pol = DtPolicy(1.e30, f0, mx, fix_dt=fix)
    s.upload(g[pre + "ic"])
    dts = []
    for _ in range(len(g[pre + "dts"])):
        s.fill_bc()
        dtn = pol(s.comp_dt(P, cfl))
        s.comp_step(P, dtn)
        pol.advance(dtn)
        dts.append(dtn)
    assert np.abs(np.array(dts) / g[pre + "dts"] - 1).max() < 1e-11
    fin = s.download()
    scale = np.maximum(np.abs(g[pre + "after"][I]).max(axis=(0, 1)), 1e-3)
    assert (np.abs(fin - g[pre + "after"])[I] / scale).max() < 1e-10
    # a Cartesian solver on this state would be a different algorithm: HLLC is refused
    with pytest.raises(Exception):
        s.comp_step(dev_params(meta, kernel_set=1)[0], dt)


def sph_arrays_fac(g, pre, meta):
    """the same arrays from pyro2_amd.mesh.patch.SphericalPolar with the 1-d factors the one-launch
    kernels rebuild them from (rowf / colf: device_geometry checks the factorisation bit for bit)"""
    from pyro2_amd.mesh import patch
    dom = g[pre + "g_domain"]
    grid = patch.SphericalPolar(int(meta[0]), int(meta[1]), ng=int(meta[2]), xmin=dom[0], xmax=dom[1],
                                ymin=dom[2], ymax=dom[3])
    geo = grid.device_geometry()
    # (the golden file's arrays come from the reference run's NumPy, whose tan / sin may differ from
    # this interpreter's in the last bit: the staged and the one-launch kernels of this test both
    # take THIS grid's arrays)
    for n in SPH_NAMES:
        assert np.allclose(geo[n], g[pre + "g_" + n], rtol=1e-14, atol=0), n
    assert "rowf" in geo and "colf" in geo
    return geo


@pytest.mark.parametrize("onek,fac", [(-1, 0), (-1, 1), (2, 0), (2, 1)])
@pytest.mark.parametrize("k", range(3))
def test_comp_spherical_one_launch_equals_staged(dev, golden, k, onek, fac):
    """(onek = -1: the tile kernel k_ctu_fused_sph, the library's choice on these small grids; 2:
    the row-marching kernel k_sph_wave of round 6.  fac: the geometry rebuilt from its 1-d factors
    instead of read from the planes.)
    SphericalPolar grid: the whole step in ONE launch (k_ctu_fused_sph: the tile kernel with
    the geometry terms -- per-cell dt / Lx, dt / Ly and the geometric source in the tracing,
    external sources with their ghost rule, CGF face pressures as gradients, area / volume
    weighted corrections and update, spherical vertex divergence, source predictor-corrector)
    against the staged spherical set (nine launches, pinned stage by stage to the oracle and
    the reference's dumps above): the WHOLE array bit for bit in the bit-faithful build, 1e-10
    in the contracted one; a run with the driver's dt policy"""
    from helpers import DtPolicy
    g = golden("comp_spherical")
    pre = f"c{k}_"
    bcs = [str(b) for b in g[pre + "bc"]]
    meta = g[pre + "meta"]
    solid = [int(b in ("reflect", "reflect-even", "reflect-odd", "dirichlet")) for b in bcs]
    nx, ny, ng = int(meta[0]), int(meta[1]), int(meta[2])
    dom = g[pre + "g_domain"]
    f0, mx = g[pre + "drv"]
    fix = 0.005 if str(g[pre + "problem"]) == "advect" else -1.0
    nsteps = len(g[pre + "dts"])
    geo = sph_arrays_fac(g, pre, meta) if fac else sph_arrays(g, pre)
    kname = "k_sph_wave" if onek == 2 else "k_ctu_fused_sph"
    staged = {}
    for fm in (0, 1):
        out = {}
        for ks in (0, onek):
            P, cfl = dev_params(meta, kernel_set=ks, riemann="CGF", solid_xl=solid[0], solid_yl=solid[2],
                                fast_math=fm)
            s = comp_state(dev, nx, ny, bcs)
            s.set_geometry(geo, dom[0], dom[2])
            s.upload(g[pre + "ic"])
            pol, dts = DtPolicy(1.e30, f0, mx, fix_dt=fix), []
            for _ in range(nsteps):
                s.fill_bc()
                dtn = pol(s.comp_dt(P, cfl))
                s.comp_step(P, dtn)
                pol.advance(dtn)
                dts.append(dtn)
            out[ks] = (s.download(), dts)
        (Ua, da), (Ub, db) = out[0], out[onek]
        staged[fm] = out[0]
        if fm == 0:
            assert da == db, (k, "dts")
            assert np.array_equal(Ua, Ub), (k, np.argwhere(Ua != Ub)[:5])
        else:
            assert np.abs(np.array(db) / np.array(da) - 1).max() < 1e-10
            scale = np.maximum(np.abs(Ua).max(axis=(0, 1)), 1e-3)
            assert (np.abs(Ub - Ua) / scale).max() < 1e-10, k
    # the next dt without a ghost fill or a reduction launch: the kernel's CFL minimum covers the
    # ghost cells of the new state (their own Lx, Ly: on this grid NOT some interior cell's
    # value) -- equal to method_compute_timestep's whole-array minimum after a fill; and the
    # caller may leave the fill to the step (fuse_fill)
    for fm in (0, 1):
        P, cfl = dev_params(meta, kernel_set=onek, riemann="CGF", solid_xl=solid[0], solid_yl=solid[2],
                            fast_math=fm, fuse_fill=1)
        P0, _ = dev_params(meta, kernel_set=0, riemann="CGF", solid_xl=solid[0], solid_yl=solid[2],
                           fast_math=fm)
        s = comp_state(dev, nx, ny, bcs)
        s.set_geometry(geo, dom[0], dom[2])
        s.upload(g[pre + "ic"])
        s.fill_bc()
        pol, dts = DtPolicy(1.e30, f0, mx, fix_dt=fix), []
        for n in range(nsteps):
            assert s.comp_dt_is_cached() == (n > 0)
            dtn = pol(s.comp_dt(P, cfl))
            s.comp_step(P, dtn)              # (no fill_bc: fuse_fill)
            pol.advance(dtn)
            dts.append(dtn)
        cached = s.comp_dt(P, cfl)
        U = s.download()
        s2 = comp_state(dev, nx, ny, bcs)
        s2.set_geometry(geo, dom[0], dom[2])
        s2.upload(U)
        s2.fill_bc()
        assert not s2.comp_dt_is_cached()
        fresh = s2.comp_dt(P0, cfl)          # k_sph_cfl over the whole filled array
        I = (slice(ng, -ng), slice(ng, -ng))
        Us, ds = staged[fm]
        if fm == 0:
            assert cached == fresh, (k, cached, fresh)
            assert dts == ds and np.array_equal(U[I], Us[I]), k
        else:
            assert abs(cached / fresh - 1) < 1e-13
            assert np.abs(np.array(dts) / np.array(ds) - 1).max() < 1e-10
    # device-side stepping (pyrohip_comp_evolve: the first CFL minimum by k_sph_cfl, then the
    # kernel's own whole-array minima and the dt policy kernel, no host round trip per step), in
    # two calls, against the steps taken one by one: dt sequence, time and the WHOLE array
    for fm in (0, 1):
        P, cfl = dev_params(meta, kernel_set=onek, riemann="CGF", solid_xl=solid[0], solid_yl=solid[2],
                            fast_math=fm)
        s = comp_state(dev, nx, ny, bcs)
        s.set_geometry(geo, dom[0], dom[2])
        s.upload(g[pre + "ic"])
        pol, dts = DtPolicy(1.e30, f0, mx, fix_dt=fix), []
        for c in (3, nsteps - 3):
            dts += list(s.comp_evolve(P, cfl, pol, c))
        s1 = comp_state(dev, nx, ny, bcs)
        s1.set_geometry(geo, dom[0], dom[2])
        s1.upload(g[pre + "ic"])
        pol1, d1 = DtPolicy(1.e30, f0, mx, fix_dt=fix), []
        for _ in range(nsteps):
            s1.fill_bc()
            dtn = pol1(s1.comp_dt(P, cfl))
            s1.comp_step(P, dtn)
            pol1.advance(dtn)
            d1.append(dtn)
        assert dts == d1 and pol.t == pol1.t and pol.n == nsteps, (k, fm)
        assert np.array_equal(s.download(), s1.download()), (k, fm)
        if fm == 0 and fix < 0:
            # tmax inside the call: the spare launches do nothing, the state is the one at tmax
            tmax = float(np.sum(d1[:3])) + 0.4 * float(d1[3])
            s = comp_state(dev, nx, ny, bcs)
            s.set_geometry(geo, dom[0], dom[2])
            s.upload(g[pre + "ic"])
            pol = DtPolicy(tmax, f0, mx)
            dts = list(s.comp_evolve(P, cfl, pol, nsteps))
            s1 = comp_state(dev, nx, ny, bcs)
            s1.set_geometry(geo, dom[0], dom[2])
            s1.upload(g[pre + "ic"])
            pol1, d1t = DtPolicy(tmax, f0, mx), []
            while pol1.t < tmax:
                s1.fill_bc()
                dtn = pol1(s1.comp_dt(P, cfl))
                s1.comp_step(P, dtn)
                pol1.advance(dtn)
                d1t.append(dtn)
            assert dts == d1t and len(dts) == 4 and pol.t == tmax == pol1.t, (k, dts, d1t)
            assert np.array_equal(s.download(), s1.download()), k
            # an invalid state handed to a call: error, nothing advances, the state stays
            from pyro2_amd._lib import ERR_STATE, PyroHipError
            bad = s1.download().copy()
            bad[ng + 5, ng + 3, 1] = -1.0
            s1.upload(bad)
            polb = DtPolicy(1.e30, f0, mx)
            polb.t, polb.n, polb.dt_old = pol1.t, pol1.n, pol1.dt_old
            with pytest.raises(PyroHipError) as ei:
                s1.comp_evolve(P, cfl, polb, 3)
            assert ei.value.code == ERR_STATE and polb.n == pol1.n and polb.t == pol1.t
            assert np.array_equal(s1.download()[ng:-ng, ng:-ng], bad[ng:-ng, ng:-ng])
    # other boundary kinds (the geometry arrays do not depend on them): a reflecting wall with
    # its even / odd variables in both directions, periodic in theta -- momenta stirred so that
    # the signs of the ghost sources matter
    rng = np.random.default_rng(11 + k)
    ic = g[pre + "ic"].copy()
    ic[:, :, 2] += 1.e-2 * ic[:, :, 0] * rng.standard_normal(ic.shape[:2])
    ic[:, :, 3] += 1.e-2 * ic[:, :, 0] * rng.standard_normal(ic.shape[:2])
    ic[:, :, 1] += 1.e-3 * ic[:, :, 0]
    for bcs2 in (("reflect", "outflow", "reflect", "reflect"), ("outflow", "reflect", "periodic", "periodic"),
                 ("reflect", "reflect", "outflow", "reflect")):
        solid2 = [int(b == "reflect") for b in bcs2]
        out = {}
        for ks in (0, onek):
            P, cfl = dev_params(meta, kernel_set=ks, riemann="CGF", solid_xl=solid2[0], solid_yl=solid2[2])
            s = comp_state(dev, nx, ny, list(bcs2))
            s.set_geometry(geo, dom[0], dom[2])
            s.upload(ic)
            pol = DtPolicy(1.e30, f0, mx, fix_dt=fix)
            for _ in range(4):
                s.fill_bc()
                dtn = pol(s.comp_dt(P, cfl))
                s.comp_step(P, dtn)
                pol.advance(dtn)
            out[ks] = s.download()
        assert np.array_equal(out[0], out[onek]), (k, bcs2, np.argwhere(out[0] != out[onek])[:5])
    # the launch count of the default really is one per step -- after the library's own fill (the
    # kernel reads ghost cells through the boundary rules); a state whose ghost cells were not
    # filled by the rules (here: nothing filled them since the last step) takes the staged set
    s.fill_bc()
    dev.prof_enable(True)
    s.comp_step(P, dts[-1])
    rep = dev.prof_report()
    assert rep.get(kname, (0, 0))[0] == 1 and "k_sph_states" not in rep
    s.comp_step(P, dts[-1])
    rep = dev.prof_report()
    dev.prof_enable(False)
    assert kname not in rep and "k_sph_states" in rep


@pytest.mark.gpu
@pytest.mark.parametrize("kset", [0, -1])
def test_comp_spherical_512_vs_oracle(hip, kset):
    """SphericalPolar Sedov at 512 x 256 (the set-up of inputs.sedov.spherical),
    12 steps with the driver's dt policy: device (the staged set, and the one-launch tile
    kernel the library picks) vs the C oracle, geometry from pyro2_amd.mesh.patch.SphericalPolar"""
    from helpers import DtPolicy
    from pyro2_amd.mesh import patch
    nx, ny, ng, gamma, cfl = 512, 256, 4, 1.4, 0.8
    grid = patch.SphericalPolar(nx, ny, ng=ng, xmin=0.1, xmax=1.0, ymin=0.785, ymax=2.355)
    geo = grid.device_geometry()
    bcs = ["reflect-odd", "outflow", "outflow", "outflow"]
    U0 = np.zeros((grid.qx, grid.qy, 4))
    U0[:, :, 0] = 1.0
    U0[:, :, 1] = 1.e-6 / (gamma - 1.0)
    U0[:, :, 1][np.asarray(grid.x2d) < 0.13] = 1.e6
    meta = [nx, ny, ng, grid.dx, grid.dy, gamma, 2, 1, 0.75, 0.85, 0.33, 0.1, 0.0, cfl]
    P, _ = dev_params(meta, kernel_set=kset, riemann="CGF", solid_xl=1, solid_yl=0)
    Po, _ = meta_to_params(meta, bcs, riemann="CGF")
    og = orc.Geom(geo, grid.xmin, grid.ymin)
    s = comp_state(hip, nx, ny, bcs)
    s.set_geometry(geo, grid.xmin, grid.ymin)
    s.upload(U0)
    Uo = U0.copy()
    pol_d, pol_o = DtPolicy(1.e30), DtPolicy(1.e30)
    for _ in range(12):
        s.fill_bc()
        dt = pol_d(s.comp_dt(P, cfl))
        s.comp_step(P, dt)
        pol_d.advance(dt)
        orc.comp_fill_bc(Uo, nx, ny, ng, bcs, gamma, 0.0, grid.dy, (0.0,) * 4)
        dto = pol_o(orc.comp_dt_geom(Uo, nx, ny, ng, og, gamma, cfl))
        assert orc.comp_step(Uo, Po, dto, geom=og)[0] == 0
        pol_o.advance(dto)
        assert abs(dt / dto - 1) < 1e-12
    U1 = s.download()
    I = (slice(ng, -ng), slice(ng, -ng))
    scale = np.maximum(np.abs(Uo[I]).max(axis=(0, 1)), 1e-3)
    assert (np.abs(U1 - Uo)[I] / scale).max() <= TOL_EXACT
    assert np.isfinite(U1[I]).all() and U1[I][:, :, 0].min() > 0


def test_bench_rank_geometry_16384(dev):
    """the slabs bench.py --gpus N cuts out of its 16384^2 grid (decomp.SlabDecomp) and the
    launch geometry the row-marching kernel takes on each of them
    (pyrohip_comp_wave_geometry, no kernel runs): on 2 / 4 / 8 ranks every rank has the same
    column strips, strip length and strip count, the first and the last strip can go first
    with the halo exchange beside the interior ones (>= 3 strips of >= ng rows), no strip is
    shorter than the ghost width, and a slab's launch still runs several rounds of resident
    wavefronts at N = 8 (36 strips of 57 rows x 293 column strips = 5 rounds: the tail and the
    8 apron rows per strip are what DESIGN 6's prediction prices).  Uneven slabs: the last strip still holds the
    ng rows a neighbour receives (a shorter one joins its predecessor), whatever the rank's
    own strip count -- the exchange protocol does not depend on it (every step posts)."""
    from pyro2_amd.decomp import SlabDecomp
    ng, cus = 4, 256
    for nranks in (1, 2, 4, 8):
        geos = []
        for rank in range(nranks):
            dec = SlabDecomp(16384, nranks, rank)
            assert dec.nx_local == 16384 // nranks and dec.i0 == rank * dec.nx_local
            geos.append(device.comp_wave_geometry(dec.nx_local, 16384, ng, cus))
        g0 = geos[0]
        assert all(g == g0 for g in geos)
        assert g0["col_strips"] == 293 and g0["slots"] == 2048
        assert g0["overlap"] == 1 and g0["row_strips"] >= 3 and g0["rows_per_strip"] >= 32
        last = 16384 // nranks - (g0["row_strips"] - 1) * g0["rows_per_strip"]
        assert last >= ng
        assert g0["wavefronts"] == g0["col_strips"] * g0["row_strips"]
        if nranks == 8:
            assert 4 * g0["slots"] <= g0["wavefronts"] <= 6 * g0["slots"]
    for nx, nranks in ((10000, 8), (16385, 4), (1250 * 3 + 1, 3)):
        for rank in range(nranks):
            dec = SlabDecomp(nx, nranks, rank)
            g = device.comp_wave_geometry(dec.nx_local, 4096, ng, cus)
            last = dec.nx_local - (g["row_strips"] - 1) * g["rows_per_strip"]
            assert ng <= last <= 2 * g["rows_per_strip"]
            assert g["overlap"] == int(g["row_strips"] >= 3 and g["rows_per_strip"] >= ng)


# (nx, ny, num_cus, comp_wave_geometry with march_rows 0, with march_rows 16, swe_wave_geometry): each as
# the tuple of the dict's values in its order, ng = 4 -- recorded on the commit in front of csrc/wave_march.h
WAVE_GEOMETRY_PINNED = [
    (8, 64, 0, (2, 8, 1, 0, 2, 2048), (2, 8, 1, 0, 2, 2048), (2, 8, 1, 0, 2, 2048)),
    (8, 64, 4, (2, 8, 1, 0, 2, 32), (2, 8, 1, 0, 2, 32), (2, 8, 1, 0, 2, 32)),
    (8, 64, 256, (2, 8, 1, 0, 2, 2048), (2, 8, 1, 0, 2, 2048), (2, 8, 1, 0, 2, 2048)),
    (8, 4096, 0, (74, 8, 1, 0, 74, 2048), (74, 8, 1, 0, 74, 2048), (71, 8, 1, 0, 71, 2048)),
    (8, 4096, 4, (74, 8, 1, 0, 74, 32), (74, 8, 1, 0, 74, 32), (71, 8, 1, 0, 71, 32)),
    (8, 4096, 256, (74, 8, 1, 0, 74, 2048), (74, 8, 1, 0, 74, 2048), (71, 8, 1, 0, 71, 2048)),
    (31, 64, 0, (2, 31, 1, 0, 2, 2048), (2, 16, 2, 0, 4, 2048), (2, 16, 2, 2, 6, 2048)),
    (31, 64, 4, (2, 31, 1, 0, 2, 32), (2, 16, 2, 0, 4, 32), (2, 16, 2, 2, 6, 32)),
    (31, 64, 256, (2, 31, 1, 0, 2, 2048), (2, 16, 2, 0, 4, 2048), (2, 16, 2, 2, 6, 2048)),
    (31, 4096, 0, (74, 31, 1, 0, 74, 2048), (74, 16, 2, 0, 148, 2048), (71, 16, 2, 71, 213, 2048)),
    (31, 4096, 4, (74, 31, 1, 0, 74, 32), (74, 16, 2, 0, 148, 32), (71, 16, 2, 0, 142, 32)),
    (31, 4096, 256, (74, 31, 1, 0, 74, 2048), (74, 16, 2, 0, 148, 2048), (71, 16, 2, 71, 213, 2048)),
    (32, 64, 0, (2, 32, 1, 0, 2, 2048), (2, 16, 2, 0, 4, 2048), (2, 16, 2, 2, 6, 2048)),
    (32, 64, 4, (2, 32, 1, 0, 2, 32), (2, 16, 2, 0, 4, 32), (2, 16, 2, 2, 6, 32)),
    (32, 64, 256, (2, 32, 1, 0, 2, 2048), (2, 16, 2, 0, 4, 2048), (2, 16, 2, 2, 6, 2048)),
    (32, 4096, 0, (74, 32, 1, 0, 74, 2048), (74, 16, 2, 0, 148, 2048), (71, 16, 2, 71, 213, 2048)),
    (32, 4096, 4, (74, 32, 1, 0, 74, 32), (74, 16, 2, 0, 148, 32), (71, 16, 2, 0, 142, 32)),
    (32, 4096, 256, (74, 32, 1, 0, 74, 2048), (74, 16, 2, 0, 148, 2048), (71, 16, 2, 71, 213, 2048)),
    (33, 64, 0, (2, 8, 4, 1, 8, 2048), (2, 16, 2, 0, 4, 2048), (2, 16, 3, 2, 8, 2048)),
    (33, 64, 4, (2, 8, 4, 1, 8, 32), (2, 16, 2, 0, 4, 32), (2, 16, 3, 2, 8, 32)),
    (33, 64, 256, (2, 8, 4, 1, 8, 2048), (2, 16, 2, 0, 4, 2048), (2, 16, 3, 2, 8, 2048)),
    (33, 4096, 0, (74, 8, 4, 1, 296, 2048), (74, 16, 2, 0, 148, 2048), (71, 16, 3, 71, 284, 2048)),
    (33, 4096, 4, (74, 15, 2, 0, 148, 32), (74, 16, 2, 0, 148, 32), (71, 17, 2, 0, 142, 32)),
    (33, 4096, 256, (74, 8, 4, 1, 296, 2048), (74, 16, 2, 0, 148, 2048), (71, 16, 3, 71, 284, 2048)),
    (64, 64, 0, (2, 8, 8, 1, 16, 2048), (2, 16, 4, 1, 8, 2048), (2, 16, 4, 2, 10, 2048)),
    (64, 64, 4, (2, 8, 8, 1, 16, 32), (2, 16, 4, 1, 8, 32), (2, 16, 4, 2, 10, 32)),
    (64, 64, 256, (2, 8, 8, 1, 16, 2048), (2, 16, 4, 1, 8, 2048), (2, 16, 4, 2, 10, 2048)),
    (64, 4096, 0, (74, 8, 8, 1, 592, 2048), (74, 16, 4, 1, 296, 2048), (71, 16, 4, 71, 355, 2048)),
    (64, 4096, 4, (74, 21, 3, 1, 222, 32), (74, 16, 4, 1, 296, 32), (71, 16, 4, 0, 284, 32)),
    (64, 4096, 256, (74, 8, 8, 1, 592, 2048), (74, 16, 4, 1, 296, 2048), (71, 16, 4, 71, 355, 2048)),
    (100, 64, 0, (2, 8, 13, 1, 26, 2048), (2, 16, 7, 1, 14, 2048), (2, 16, 7, 2, 16, 2048)),
    (100, 64, 4, (2, 8, 13, 1, 26, 32), (2, 16, 7, 1, 14, 32), (2, 16, 7, 2, 16, 32)),
    (100, 64, 256, (2, 8, 13, 1, 26, 2048), (2, 16, 7, 1, 14, 2048), (2, 16, 7, 2, 16, 2048)),
    (100, 4096, 0, (74, 8, 13, 1, 962, 2048), (74, 16, 7, 1, 518, 2048), (71, 16, 7, 71, 568, 2048)),
    (100, 4096, 4, (74, 33, 3, 1, 222, 32), (74, 16, 7, 1, 518, 32), (71, 25, 4, 0, 284, 32)),
    (100, 4096, 256, (74, 8, 13, 1, 962, 2048), (74, 16, 7, 1, 518, 2048), (71, 16, 7, 71, 568, 2048)),
    (257, 64, 0, (2, 8, 32, 1, 64, 2048), (2, 16, 16, 1, 32, 2048), (2, 16, 17, 2, 36, 2048)),
    (257, 64, 4, (2, 16, 16, 1, 32, 32), (2, 16, 16, 1, 32, 32), (2, 17, 16, 0, 32, 32)),
    (257, 64, 256, (2, 8, 32, 1, 64, 2048), (2, 16, 16, 1, 32, 2048), (2, 16, 17, 2, 36, 2048)),
    (257, 4096, 0, (74, 10, 26, 1, 1924, 2048), (74, 16, 16, 1, 1184, 2048), (71, 16, 17, 71, 1278, 2048)),
    (257, 4096, 4, (74, 85, 3, 1, 222, 32), (74, 16, 16, 1, 1184, 32), (71, 65, 4, 0, 284, 32)),
    (257, 4096, 256, (74, 10, 26, 1, 1924, 2048), (74, 16, 16, 1, 1184, 2048), (71, 16, 17, 71, 1278, 2048)),
    (1024, 64, 0, (2, 8, 128, 1, 256, 2048), (2, 16, 64, 1, 128, 2048), (2, 16, 64, 2, 130, 2048)),
    (1024, 64, 4, (2, 64, 16, 1, 32, 32), (2, 16, 64, 1, 128, 32), (2, 64, 16, 0, 32, 32)),
    (1024, 64, 256, (2, 8, 128, 1, 256, 2048), (2, 16, 64, 1, 128, 2048), (2, 16, 64, 2, 130, 2048)),
    (1024, 4096, 0, (74, 38, 27, 1, 1998, 2048), (74, 16, 64, 1, 4736, 2048), (71, 37, 28, 60, 2048, 2048)),
    (1024, 4096, 4, (74, 114, 9, 1, 666, 32), (74, 16, 64, 1, 4736, 32), (71, 114, 9, 0, 639, 32)),
    (1024, 4096, 256, (74, 38, 27, 1, 1998, 2048), (74, 16, 64, 1, 4736, 2048), (71, 37, 28, 60, 2048, 2048)),
    (1792, 64, 0, (2, 8, 224, 1, 448, 2048), (2, 16, 112, 1, 224, 2048), (2, 16, 112, 2, 226, 2048)),
    (1792, 64, 4, (2, 112, 16, 1, 32, 32), (2, 16, 112, 1, 224, 32), (2, 112, 16, 0, 32, 32)),
    (1792, 64, 256, (2, 8, 224, 1, 448, 2048), (2, 16, 112, 1, 224, 2048), (2, 16, 112, 2, 226, 2048)),
    (1792, 4096, 0, (74, 67, 27, 1, 1998, 2048), (74, 16, 112, 1, 8288, 2048), (71, 64, 28, 60, 2048, 2048)),
    (1792, 4096, 4, (74, 112, 16, 1, 1184, 32), (74, 16, 112, 1, 8288, 32), (71, 138, 13, 0, 923, 32)),
    (1792, 4096, 256, (74, 67, 27, 1, 1998, 2048), (74, 16, 112, 1, 8288, 2048), (71, 64, 28, 60, 2048, 2048)),
    (2048, 64, 0, (2, 8, 256, 1, 512, 2048), (2, 16, 128, 1, 256, 2048), (2, 16, 128, 2, 258, 2048)),
    (2048, 64, 4, (2, 128, 16, 1, 32, 32), (2, 16, 128, 1, 256, 32), (2, 128, 16, 0, 32, 32)),
    (2048, 64, 256, (2, 8, 256, 1, 512, 2048), (2, 16, 128, 1, 256, 2048), (2, 16, 128, 2, 258, 2048)),
    (2048, 4096, 0, (74, 76, 27, 1, 1998, 2048), (74, 16, 128, 1, 9472, 2048), (71, 74, 28, 60, 2048, 2048)),
    (2048, 4096, 4, (74, 128, 16, 1, 1184, 32), (74, 16, 128, 1, 9472, 32), (71, 114, 18, 0, 1278, 32)),
    (2048, 4096, 256, (74, 76, 27, 1, 1998, 2048), (74, 16, 128, 1, 9472, 2048), (71, 74, 28, 60, 2048, 2048)),
    (3072, 64, 0, (2, 8, 384, 1, 768, 2048), (2, 16, 192, 1, 384, 2048), (2, 16, 192, 2, 386, 2048)),
    (3072, 64, 4, (2, 32, 96, 1, 192, 32), (2, 16, 192, 1, 384, 32), (2, 32, 96, 0, 192, 32)),
    (3072, 64, 256, (2, 8, 384, 1, 768, 2048), (2, 16, 192, 1, 384, 2048), (2, 16, 192, 2, 386, 2048)),
    (3072, 4096, 0, (74, 114, 27, 1, 1998, 2048), (74, 16, 192, 1, 14208, 2048), (71, 110, 28, 60, 2048, 2048)),
    (3072, 4096, 4, (74, 140, 22, 1, 1628, 32), (74, 16, 192, 1, 14208, 32), (71, 140, 22, 0, 1562, 32)),
    (3072, 4096, 256, (74, 114, 27, 1, 1998, 2048), (74, 16, 192, 1, 14208, 2048), (71, 110, 28, 60, 2048, 2048)),
    (4096, 64, 0, (2, 8, 512, 1, 1024, 2048), (2, 16, 256, 1, 512, 2048), (2, 16, 256, 2, 514, 2048)),
    (4096, 64, 4, (2, 43, 96, 1, 192, 32), (2, 16, 256, 1, 512, 32), (2, 32, 128, 0, 256, 32)),
    (4096, 64, 256, (2, 8, 512, 1, 1024, 2048), (2, 16, 256, 1, 512, 2048), (2, 16, 256, 2, 514, 2048)),
    (4096, 4096, 0, (74, 152, 27, 1, 1998, 2048), (74, 16, 256, 1, 18944, 2048), (71, 147, 28, 60, 2048, 2048)),
    (4096, 4096, 4, (74, 128, 32, 1, 2368, 32), (74, 16, 256, 1, 18944, 32), (71, 152, 27, 0, 1917, 32)),
    (4096, 4096, 256, (74, 152, 27, 1, 1998, 2048), (74, 16, 256, 1, 18944, 2048), (71, 147, 28, 60, 2048, 2048)),
    (8192, 64, 0, (2, 8, 1024, 1, 2048, 2048), (2, 16, 512, 1, 1024, 2048), (2, 16, 512, 2, 1026, 2048)),
    (8192, 64, 4, (2, 64, 128, 1, 256, 32), (2, 16, 512, 1, 1024, 32), (2, 57, 144, 0, 288, 32)),
    (8192, 64, 256, (2, 8, 1024, 1, 2048, 2048), (2, 16, 512, 1, 1024, 2048), (2, 16, 512, 2, 1026, 2048)),
    (8192, 4096, 0, (74, 50, 164, 1, 12136, 2048), (74, 16, 512, 1, 37888, 2048), (71, 41, 200, 0, 14200, 2048)),
    (8192, 4096, 4, (74, 152, 54, 1, 3996, 32), (74, 16, 512, 1, 37888, 32), (71, 152, 54, 0, 3834, 32)),
    (8192, 4096, 256, (74, 50, 164, 1, 12136, 2048), (74, 16, 512, 1, 37888, 2048), (71, 41, 200, 0, 14200, 2048)),
    (16384, 64, 0, (2, 16, 1024, 1, 2048, 2048), (2, 16, 1024, 1, 2048, 2048), (2, 16, 1024, 0, 2048, 2048)),
    (16384, 64, 4, (2, 79, 208, 1, 416, 32), (2, 16, 1024, 1, 2048, 32), (2, 64, 256, 0, 512, 32)),
    (16384, 64, 256, (2, 16, 1024, 1, 2048, 2048), (2, 16, 1024, 1, 2048, 2048), (2, 16, 1024, 0, 2048, 2048)),
    (16384, 4096, 0, (74, 66, 249, 1, 18426, 2048), (74, 16, 1024, 1, 75776, 2048), (71, 57, 288, 0, 20448, 2048)),
    (16384, 4096, 4, (74, 152, 108, 1, 7992, 32), (74, 16, 1024, 1, 75776, 32), (71, 158, 104, 0, 7384, 32)),
    (16384, 4096, 256, (74, 66, 249, 1, 18426, 2048), (74, 16, 1024, 1, 75776, 2048), (71, 57, 288, 0, 20448, 2048)),
]


def test_wave_geometry_pinned():
    """the launch geometry of the row-marching compressible and shallow-water kernels (no kernel
    runs) is what it was before the strip rules moved into csrc/wave_march.h (wave_strip_rows,
    wave_strip_count, wave_fill_extra): strips from 8 rows to 16384, a column strip or 74 of them,
    the default / 4 / 256 compute units, the library's strip length and a caller's 16 rows"""
    from conftest import _get_ctx
    _get_ctx("emu")
    assert len(WAVE_GEOMETRY_PINNED) == 14 * 2 * 3
    for nx, ny, cus, c0, c16, sw in WAVE_GEOMETRY_PINNED:
        assert tuple(device.comp_wave_geometry(nx, ny, 4, cus, 0).values()) == c0, (nx, ny, cus)
        assert tuple(device.comp_wave_geometry(nx, ny, 4, cus, 16).values()) == c16, (nx, ny, cus)
        assert tuple(device.swe_wave_geometry(nx, ny, 4, cus).values()) == sw, (nx, ny, cus)


@pytest.mark.parametrize("riemann", ["HLLC", "CGF", "HLLC_lm"])
@pytest.mark.parametrize("nx,ny,grav,lim,flat,rows", [
    (40, 130, 0.0, 2, 1, 0), (33, 57, -1.5, 2, 1, 7), (64, 64, -1.5, 1, 0, 16)])
def test_rk_rhs_one_launch_equals_staged(dev, riemann, nx, ny, grav, lim, flat, rows):
    """compressible_rk's right-hand side by ONE launch of the row-marching kernel's
    method-of-lines instance (k_ctu_wave<.., MOL>: piecewise linear face states, no transverse
    problems, k = -div F + S stored) against the staged k_prim / k_xi / k_rk_states / k_rk_flux /
    k_rk_rhs: every solver, gravity, both reconstructions, strips of 7 / 16 rows and the
    library's choice, a density floor that bites (clean_state works in place: the stage state
    is compared too) -- bit for bit in the bit-faithful build"""
    rng = np.random.default_rng(5)
    ic = np.zeros((nx + 8, ny + 8, 4))
    x = np.arange(nx + 8)[:, None] / nx
    y = np.arange(ny + 8)[None, :] / ny
    ic[..., 0] = 1.0 + 0.5 * np.sin(7 * x) * np.cos(5 * y) + 0.1 * rng.random((nx + 8, ny + 8))
    ic[..., 2] = 0.4 * np.cos(3 * x + y)
    ic[..., 3] = -0.3 * np.sin(4 * y - x)
    ic[..., 1] = 2.5 + 5.0 * np.exp(-40 * ((x - 0.5) ** 2 + (y - 0.5) ** 2)) + \
        0.5 * (ic[..., 2] ** 2 + ic[..., 3] ** 2) / ic[..., 0]
    bcs = [["outflow", "outflow", "reflect-even", "outflow"]] * 3 + [["outflow", "outflow", "reflect-odd", "outflow"]]
    out = {}
    for ks in (0, 2):
        P = device.make_comp_params(1.0 / nx, 1.0 / ny, fast_math=0, kernel_set=ks, riemann=riemann,
                                    grav=grav, limiter=lim, use_flattening=flat, march_rows=rows,
                                    small_dens=1.05)
        s = device.DeviceState(dev, nx, ny, 4, bcs)
        s.upload(ic)
        s.fill_bc()
        k = device.DeviceState(dev, nx, ny, 4, [["outflow"] * 4] * 8)
        k.upload(np.zeros((nx + 8, ny + 8, 8)))
        s.comp_rk_rhs(P, k, 1)
        out[ks] = (k.download()[4:-4, 4:-4, 4:8].copy(), s.download().copy())
    assert np.array_equal(out[0][0], out[2][0])
    assert np.array_equal(out[0][1], out[2][1])
    assert (out[2][1][4:-4, 4:-4, 0] >= 1.05).all() and (ic[4:-4, 4:-4, 0] < 1.05).any()


RK_BCS = [("outflow", "outflow", "outflow", "outflow"), ("reflect", "reflect", "periodic", "periodic"),
          ("periodic", "periodic", "reflect", "outflow")]


def _rk_random_state(nx, ny, seed):
    rng = np.random.default_rng(seed)
    ng = 4
    x = np.arange(nx + 2 * ng)[:, None] / nx
    y = np.arange(ny + 2 * ng)[None, :] / ny
    U = np.zeros((nx + 2 * ng, ny + 2 * ng, 4))
    U[..., 0] = 1.0 + 0.3 * np.sin(5 * x) * np.cos(3 * y) + 0.05 * rng.random(U.shape[:2])
    U[..., 2] = U[..., 0] * 0.3 * np.cos(4 * x + y)
    U[..., 3] = U[..., 0] * -0.2 * np.sin(3 * y - 2 * x)
    U[..., 1] = (1.0 + 0.5 * np.cos(2 * x) * np.sin(2 * y)) / 0.4 + 0.5 * (U[..., 2] ** 2 + U[..., 3] ** 2) / U[..., 0]
    return U


RK_CASES = [(m, b, 40, 130, 0.0, "HLLC") for m in ("RK2", "TVD2", "TVD3", "RK4") for b in RK_BCS] + \
           [("RK4", RK_BCS[1], 23, 61, -0.7, "CGF"), ("TVD3", RK_BCS[2], 23, 61, -0.7, "CGF"),
            ("RK2", RK_BCS[0], 23, 61, -0.7, "HLLC_lm")]


@pytest.mark.parametrize("method,bcs,nx,ny,grav,riemann", RK_CASES)
def test_rk_step_in_one_call_equals_stage_by_stage(dev, method, bcs, nx, ny, grav, riemann):
    """pyrohip_comp_rk_step (the stage states built at load from y_0 and the earlier increments,
    ghost cells through the boundary rules, the final update + CFL minimum in the last stage:
    k_ctu_wave<.., MOL, false, RKF>) against the stage-by-stage path -- lincomb, ghost fill,
    pyrohip_comp_rk_rhs, final lincomb, comp_rk_dt -- three steps: the bit-faithful build bit for
    bit (interior AND ghost cells), every method, boundary kinds incl. odd reflections, several
    column strips / row chunks"""
    from helpers import RK_TABLEAU
    ng = 4
    meta = [nx, ny, ng, 1.0 / nx, 1.5 / ny, 1.4, 2, 1, 0.75, 0.85, 0.33, 0.1, grav, 0.8]
    solid = [int(b == "reflect") for b in bcs]
    a, b = RK_TABLEAU[method]
    ns = len(b)
    U0 = _rk_random_state(nx, ny, nx * ny + ns)
    # (the contracted build defers the last increment of a stage start to the row's consumption:
    # on the emulator its arithmetic is the bit-faithful one, so it is held to the same identity)
    for fast in ((0, 1) if method in ("RK4", "TVD3") else (0,)):
        _rk_one_call_vs_stages(dev, meta, riemann, solid, bcs, a, b, ns, U0, nx, ny, ng, fast)


def _rk_one_call_vs_stages(dev, meta, riemann, solid, bcs, a, b, ns, U0, nx, ny, ng, fast):
    P, cfl = dev_params(meta, kernel_set=2, riemann=riemann, solid_xl=solid[0], solid_yl=solid[2], march_rows=16,
                        fast_math=fast)
    out = {}
    for fused in (0, 1):
        s = comp_state(dev, nx, ny, list(bcs))
        y = comp_state(dev, nx, ny, list(bcs))
        kst = device.DeviceState(dev, nx, ny, ng, [["outflow"] * 4] * (4 * ns))
        s.upload(U0)
        if fused:
            assert s.comp_rk_can_fuse(P, kst, ns)
        dts = []
        for n in range(3):
            s.fill_bc()
            dt = 0.3 * s.comp_rk_dt(P, cfl)
            dts.append(dt)
            if fused:
                s.comp_rk_step(P, kst, dt, a, b)
                continue
            for st in range(ns):
                cur = s
                if st:
                    y.lincomb(s, kst, [dt * a[st][j] for j in range(st)])
                    y.fill_bc()
                    cur = y
                cur.comp_rk_rhs(P, kst, st)
            s.lincomb(s, kst, [dt * b[st] for st in range(ns)])
        out[fused] = (s.download(), dts)
    if dev.kind == "emu":
        assert out[0][1] == out[1][1]
        assert np.array_equal(out[0][0], out[1][0]), np.argwhere(out[0][0] != out[1][0])[:5]
    else:
        tol = TOL_FAST if fast else TOL_EXACT
        assert np.abs(np.array(out[1][1]) / np.array(out[0][1]) - 1).max() <= tol
        assert elementwise_close(out[1][0], out[0][0], tol)


def elementwise_close(a, b, tol):
    scale = np.maximum(np.abs(b).max(axis=(0, 1)), 1e-3)
    return bool((np.abs(a - b) / scale).max() <= tol)


@pytest.mark.parametrize("method", ["RK4", "TVD3"])
def test_rk_evolve_on_device_equals_single_steps(dev, method):
    """pyrohip_comp_rk_evolve (dt policy on the device between the steps, tmax inside the call)
    against the same steps taken one by one from the host: dt sequence, time, state -- exact"""
    from helpers import RK_TABLEAU
    nx, ny, ng = 36, 70, 4
    meta = [nx, ny, ng, 1.0 / nx, 1.0 / ny, 1.4, 2, 1, 0.75, 0.85, 0.33, 0.1, 0.0, 0.8]
    bcs = ["outflow", "outflow", "periodic", "periodic"]
    P, cfl = dev_params(meta, kernel_set=2, march_rows=16)
    a, b = RK_TABLEAU[method]
    ns = len(b)
    U0 = _rk_random_state(nx, ny, 5)
    res = []
    for tmax in (1.e30, None):
        s1 = comp_state(dev, nx, ny, bcs)
        k1 = device.DeviceState(dev, nx, ny, ng, [["outflow"] * 4] * (4 * ns))
        s1.upload(U0)
        if tmax is None:      # ends inside the fifth step of the first run
            tmax = sum(res[0][0][:4]) + 0.4 * res[0][0][4]
        pol1 = DtPolicy(tmax)
        d1 = []
        while pol1.t < tmax and pol1.n < 6:
            s1.fill_bc()
            dt = pol1(s1.comp_rk_dt(P, cfl))
            s1.comp_rk_step(P, k1, dt, a, b)
            pol1.advance(dt)
            d1.append(dt)
        s = comp_state(dev, nx, ny, bcs)
        k = device.DeviceState(dev, nx, ny, ng, [["outflow"] * 4] * (4 * ns))
        s.upload(U0)
        pol = DtPolicy(tmax)
        dts = list(s.comp_rk_evolve(P, k, a, b, cfl, pol, 2))
        dts += list(s.comp_rk_evolve(P, k, a, b, cfl, pol, 4))
        assert dts == d1 and pol.t == pol1.t and pol.n == pol1.n, (dts, d1)
        # the whole array, ghost cells included -- also where tmax ended the run inside a call (the
        # iterations past it keep filling frames; the library rebuilds the final state's: ADVICE r5)
        assert np.array_equal(s.download(), s1.download())
        # the next dt comes from the cached minimum: equal to a fresh reduction over the filled state
        cached = s.comp_rk_dt(P, cfl)
        s1.fill_bc()
        s1.upload(s1.download())          # (drops the cache)
        assert cached == s1.comp_rk_dt(P, cfl)
        res.append((d1,))


@pytest.mark.parametrize("fast", [0, 1])
def test_comp_wave_short_tail_of_a_many_round_launch(dev, fast):
    """launches of four and more rounds of resident wavefronts cut the row strips of their last round's worth of
    units in two and deal them to the ends of the eight XCD queues (comp_wave.hip: wave_short_tail).  The emulated
    device has 32 wavefront slots: 512 x 224 cells in 16-row strips are 4 column x 32 row strips = four rounds -> 24
    long + 16 short row strips.  Three steps (host-stepped and on the device) against the tile kernel: every cell
    updated exactly once, bit for bit in the bit-faithful build (the contracted one computes a cell the same way
    whatever strip it sits in: the two kernels differ by their algebra, 1e-10)"""
    if dev.kind == "hip":
        pytest.skip("a 512 x 224 grid is one round on this device (the bench-size tests cover its many-round launches)")
    nx, ny, ng = 512, 224, 4
    meta = [nx, ny, ng, 1.0 / nx, 1.0 / ny, 1.4, 2, 1, 0.75, 0.85, 0.33, 0.1, 0.0, 0.8]
    bcs = ["outflow", "reflect", "periodic", "periodic"]
    U0 = _rk_random_state(nx, ny, 11)
    ref, dref, _ = device_comp_run(dev, U0, meta, bcs, 1.0, 3, kernel_set=1, fast_math=fast)
    got, dgot, _ = device_comp_run(dev, U0, meta, bcs, 1.0, 3, kernel_set=2, march_rows=16, fast_math=fast)
    P, cfl = dev_params(meta, kernel_set=2, march_rows=16, fast_math=fast)
    s = comp_state(dev, nx, ny, bcs)
    s.upload(U0)
    pol = DtPolicy(1.0)
    dts = list(s.comp_evolve(P, cfl, pol, 3))
    onb = s.download()
    if fast == 0:
        assert list(dgot) == list(dref) == dts
        assert np.array_equal(got[ng:-ng, ng:-ng], ref[ng:-ng, ng:-ng])
        assert np.array_equal(onb[ng:-ng, ng:-ng], ref[ng:-ng, ng:-ng])
    else:
        assert elementwise_err(got[ng:-ng, ng:-ng], ref[ng:-ng, ng:-ng], comp_floors(ref[ng:-ng, ng:-ng])) <= 1e-10
        assert np.array_equal(onb[ng:-ng, ng:-ng], got[ng:-ng, ng:-ng])


@pytest.mark.parametrize("solver", ["ctu_tile", "ctu_wave", "rk"])
def test_evolve_starts_from_the_cached_minimum_only_for_an_untouched_state(dev, solver):
    """a device-side run starts from the CFL minimum the previous call's last step left (no pass over the
    whole array) -- only while that minimum still describes the state: after an upload, or with another
    dx, the call reduces the array again.  Second call on a state written in between / with other
    parameters against a fresh state object that has no history: dt sequence and state bit for bit"""
    from helpers import RK_TABLEAU
    nx, ny, ng = 36, 70, 4
    meta = [nx, ny, ng, 1.0 / nx, 1.0 / ny, 1.4, 2, 1, 0.75, 0.85, 0.33, 0.1, 0.0, 0.8]
    bcs = ["outflow", "outflow", "periodic", "periodic"]
    kw = {"ctu_tile": dict(kernel_set=1), "ctu_wave": dict(kernel_set=2, march_rows=16),
          "rk": dict(kernel_set=2, march_rows=16)}[solver]
    P, cfl = dev_params(meta, **kw)
    meta2 = list(meta)
    meta2[3] = 0.5 / nx
    P2, _ = dev_params(meta2, **kw)
    a, b = RK_TABLEAU["RK4"]

    def run(s, k, PP, pol, n):
        if solver == "rk":
            return list(s.comp_rk_evolve(PP, k, a, b, cfl, pol, n))
        return list(s.comp_evolve(PP, cfl, pol, n))

    def fresh(U):
        s = comp_state(dev, nx, ny, bcs)
        k = device.DeviceState(dev, nx, ny, ng, [["outflow"] * 4] * 16) if solver == "rk" else None
        s.upload(U)
        return s, k

    U0, U1 = _rk_random_state(nx, ny, 5), _rk_random_state(nx, ny, 6)
    for what in ("upload", "dx"):
        s, k = fresh(U0)
        pol = DtPolicy(1.e30)
        run(s, k, P, pol, 3)
        if what == "upload":
            s.upload(U1)
            Ustart, PP = U1, P
        else:
            Ustart, PP = s.download(), P2
        polb = DtPolicy(1.e30)
        polb.t, polb.n, polb.dt_old = pol.t, pol.n, pol.dt_old
        d2 = run(s, k, PP, pol, 3)
        sf, kf = fresh(Ustart)
        df = run(sf, kf, PP, polb, 3)
        assert d2 == df, (what, d2, df)
        assert np.array_equal(s.download()[ng:-ng, ng:-ng], sf.download()[ng:-ng, ng:-ng]), what


@pytest.mark.parametrize("kset", KSETS)
def test_comp_negative_zero_momentum_traces_like_the_reference(dev, kset):
    """the tracing takes copysign(1, u) (interface.py:198-201): a cell whose x-momentum is exactly
    -0.0 -- e.g. the odd reflection of a gas at rest -- sends its shear / entropy waves to the LOWER
    face.  The bit-faithful GPU quotient (reciprocal + Markstein correction) returned +0 for -0 / rho
    (found in round 5 through the shallow-water build); hydro.h: pvel keeps the sign.  One step of
    a sheared state at rest in x with -0.0 / +0.0 bands, against the oracle"""
    from helpers import oracle_comp_run
    nx, ny, ng = 24, 20, 4
    meta = [nx, ny, ng, 1.0 / nx, 1.0 / ny, 1.4, 2, 1, 0.75, 0.85, 0.33, 0.1, 0.0, 0.8]
    bcs = ["periodic"] * 4
    x = np.arange(nx + 2 * ng)[:, None] / nx
    y = np.arange(ny + 2 * ng)[None, :] / ny
    U = np.zeros((nx + 2 * ng, ny + 2 * ng, 4))
    U[..., 0] = 1.0 + 0.2 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y)
    v = 0.3 * np.sin(2 * np.pi * x)                   # shear: d v / d x != 0
    U[..., 3] = U[..., 0] * v
    U[..., 2] = np.where((np.arange(nx + 2 * ng) % 4 < 2)[:, None], -0.0, 0.0)
    U[..., 1] = 2.5 + 0.5 * U[..., 0] * v * v
    assert np.signbit(U[..., 2]).any() and not np.signbit(U[..., 2]).all()
    Uo, dto, _ = oracle_comp_run(U, meta, bcs, 1.0, 1, init_tstep_factor=1.0)
    Ud, dts, _ = _one_full_step(dev, U, meta, bcs, kset)
    tol = 0.0 if dev.kind == "emu" else 1e-13
    assert max_rel_err(dts, dto) <= tol
    for n in range(4):
        assert max_rel_err(Ud[4:-4, 4:-4, n], Uo[4:-4, 4:-4, n]) <= tol, n
    # the sign of the zero matters: with +0.0 everywhere the step is a different one
    U2 = U.copy()
    U2[..., 2] = 0.0
    Uo2, _, _ = oracle_comp_run(U2, meta, bcs, 1.0, 1, init_tstep_factor=1.0)
    assert np.abs(Uo2 - Uo)[4:-4, 4:-4].max() > 1e-9


def _one_full_step(dev, U, meta, bcs, kset):
    """one step with the full CFL time step (no init_tstep_factor)"""
    P, cfl = dev_params(meta, **kset_kw(kset))
    s = comp_state(dev, int(meta[0]), int(meta[1]), bcs)
    s.upload(U)
    s.fill_bc()
    dt = s.comp_dt(P, cfl)
    s.comp_step(P, dt)
    return s.download(), np.array([dt]), dt


def test_comp_wave_oddly_reflected_density(dev):
    """A boundary named `reflect-odd` reflects EVERY variable oddly (the reference's
    inputs.sedov.spherical does that at r = 0): the ghost cells hold a negative density and energy,
    the faces between them are no gas at all -- roots of negative numbers, which the solvers' floors
    (fmax(floor, NaN) = floor, as Python's max() in the reference) absorb, and what they feed is never
    stored -- on the spherical grid, where that face has no area.  On a Cartesian grid the flux of
    the boundary face itself is such a non-gas problem and enters the first interior row: the
    reference's result there is whatever its arithmetic makes of it, and only the bit-faithful build
    can reproduce that.  The row-marching kernel (kernel_set 2) against the staged set (0) on such a
    grid: bit-identical in the bit-faithful build; the contracted build -- compiled with
    -fno-honor-nans, round 6 -- must stay finite and valid (its floors absorb the NaN roots as well)
    and close (1e-7 measured; the problem is ill-conditioned at the boundary rows, not the build)."""
    nx, ny, ng = 96, 120, 4
    bcs = ["reflect-odd", "outflow", "reflect-odd", "outflow"]
    dx, dy = 1.0 / nx, 1.0 / ny
    meta = [nx, ny, ng, dx, dy, 1.4, 2, 1, 0.75, 0.85, 0.33, 0.1, 0.0, 0.8]
    x = (np.arange(nx + 2 * ng) - ng + 0.5) * dx
    y = (np.arange(ny + 2 * ng) - ng + 0.5) * dy
    X, Y = np.meshgrid(x, y, indexing="ij")
    U0 = np.zeros((nx + 2 * ng, ny + 2 * ng, 4))
    U0[..., 0] = 1.0 + 0.1 * np.sin(5 * X) * np.cos(3 * Y)
    U0[..., 1] = 1.e-5 / 0.4
    U0[..., 1][np.hypot(X - 0.06, Y - 0.08) < 0.05] = 10.0 / 0.4      # a blast next to the two odd sides
    out = {}
    for fm, ks in ((0, 0), (0, 2), (1, 2)):
        P, cfl = dev_params(meta, kernel_set=ks, fast_math=fm)
        s = comp_state(dev, nx, ny, bcs)
        s.upload(U0)
        pol, dts = DtPolicy(1.e30), []
        for _ in range(12):
            s.fill_bc()
            dtn = pol(s.comp_dt(P, cfl))
            s.comp_step(P, dtn)
            pol.advance(dtn)
            dts.append(dtn)
        out[fm, ks] = (s.download()[ng:-ng, ng:-ng], dts)
    (Ua, da), (Ub, db), (Uc, dc) = out[0, 0], out[0, 2], out[1, 2]
    assert np.isfinite(Ua).all() and Ua[..., 0].min() > 0
    assert da == db and np.array_equal(Ua, Ub), np.argwhere(Ua != Ub)[:5]
    assert np.isfinite(Uc).all() and Uc[..., 0].min() > 0
    assert np.abs(np.array(dc) / np.array(da) - 1).max() < 1e-6
    fl = comp_floors(Ua)
    for v in range(4):
        assert elementwise_err(Uc[..., v], Ua[..., v], fl[v]) < 1e-5, v
