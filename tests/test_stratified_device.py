"""Device-side stepping of the stratified atmospheres: hse / ambient y sides,
gravity, the heating profile and the sponge inside pyrohip_comp_evolve.  The loop's one fill
launch (k_fill_frame2_user: frames of both buffers, the hse corner rule, the CFL minimum of the
frame), the sponge behind the step (k_sponge_run) and the policy that takes the minimum of both
are held to the same steps taken singly -- fill_bc, comp_dt, the driver's policy, comp_step --
bit for bit: every comparison between the two is np.array_equal / ==."""
import numpy as np
import pytest

from helpers import DtPolicy
from pyro2_amd import _lib, device
from test_device_compressible import TOL_EXACT, comp_state, dev_params

NG = 4
BIG = 1.e30


# ---- states from the recorded reference runs ---------------------------------------------------

def _case(golden, fixture, k):
    """-> (key prefix, fixture, side kinds, keywords of the step parameters)"""
    g = golden(fixture)
    pre = f"c{k}_"
    bcs = [str(b) for b in g[pre + "bc"]]
    solid = [int(b == "reflect") for b in bcs]
    kw = dict(solid_xl=solid[0], solid_yl=solid[2])
    if fixture == "comp_hse":
        kw["riemann"] = "CGF" if k == 1 else "HLLC"      # as test_comp_hse_ambient_runs assigns them
    else:
        sp = g[pre + "sponge"]
        kw.update(small_dens=float(g[pre + "small_dens"]), heat_rate=float(g[pre + "e_rate"]),
                  sponge=tuple(sp[1:]) if sp[0] else None)
    return pre, g, bcs, kw


def _state(dev, g, pre, bcs, ic=None):
    meta = g[pre + "meta"]
    s = comp_state(dev, int(meta[0]), int(meta[1]), bcs)
    if any(b in ("hse", "ambient") for b in bcs):
        s.set_user_bc(meta[5], meta[12], meta[4], g[pre + "ambient"])
    if pre + "prof" in g.files:
        s.set_heating(g[pre + "prof"])
    s.upload(np.nan_to_num(g[pre + "ic"]) if ic is None else ic)
    return s


def _singly(s, P, cfl, pol, n):
    """n iterations of Pyro.single_step: fill, CFL step, the driver's policy, the step"""
    dts = []
    for _ in range(n):
        if pol.t >= pol.tmax:
            break
        s.fill_bc()
        dt = pol(s.comp_dt(P, cfl))
        s.comp_step(P, dt)
        pol.advance(dt)
        dts.append(dt)
    return dts


def _same_policy(a, b):
    assert (a.t, a.n, a.dt_old) == (b.t, b.n, b.dt_old)


CASES = [("comp_hse", 0), ("comp_hse", 1), ("comp_hse", 2), ("comp_hse", 3),
         ("comp_heating", 1), ("comp_heating", 2)]
_REF = {}


def _steps(dev, g, pre, fixture, k):
    # (the emulated backend cuts the runs as the tests of the same fixtures do; c2 of comp_hse
    # runs until the CFL limit, whose minimum sits in the hse ghost rows, has taken over)
    if dev.kind == "hip":
        return len(g[pre + "dts"])
    return 9 if (fixture, k) == ("comp_hse", 2) else 5


def _reference(dev, golden, fixture, k, fm):
    key = (dev.kind, fixture, k, fm)
    if key not in _REF:
        pre, g, bcs, kw = _case(golden, fixture, k)
        P, cfl = dev_params(g[pre + "meta"], kernel_set=-1, fast_math=fm, **kw)
        s = _state(dev, g, pre, bcs)
        f0, mx = g[pre + "drv"]
        pol = DtPolicy(BIG, f0, mx)
        dts = _singly(s, P, cfl, pol, _steps(dev, g, pre, fixture, k))
        U = s.download()
        U.setflags(write=False)
        _REF[key] = (dts, U, pol, s.comp_dt_is_cached())
    return _REF[key]


@pytest.mark.parametrize("fm", [0, 1])
@pytest.mark.parametrize("fixture,k", CASES)
def test_recorded_runs_through_the_loop(dev, golden, fixture, k, fm):
    """the recorded hse / ambient / heating / sponge runs in ONE comp_evolve call and in two (cut
    at an odd step count: buffer parity and the kept minimum cross a call boundary): state with
    its ghost frame, dt sequence, t, n, dt_old as the single steps of the same build leave them,
    exactly; the bit-faithful build also against the recorded dts / final at the tolerances of
    test_comp_hse_ambient_runs (TOL_EXACT * nsteps) and test_comp_problem_sources (dts 1e-12,
    state + 1e-14 for the sponge's cos())"""
    pre, g, bcs, kw = _case(golden, fixture, k)
    meta = g[pre + "meta"]
    P, cfl = dev_params(meta, kernel_set=-1, fast_math=fm, **kw)
    dref, Uref, pref, cached_ref = _reference(dev, golden, fixture, k, fm)
    n = len(dref)
    f0, mx = g[pre + "drv"]
    for chunks in ((n,), (3, n - 3)):
        s = _state(dev, g, pre, bcs)
        pol, dts = DtPolicy(BIG, f0, mx), []
        for c in chunks:
            dts += [float(x) for x in s.comp_evolve(P, cfl, pol, c)]
        assert dts == dref, chunks
        assert np.array_equal(s.download(), Uref), chunks
        _same_policy(pol, pref)
        assert s.comp_dt_is_cached() == cached_ref
    if fm:
        return
    # the recorded run (the CGF case holds one face where the reference's libm pow is an ulp
    # from x * x: test_comp_hse_ambient_runs compares it with the oracle, not with the record)
    sponge = kw.get("sponge") is not None
    if (fixture, k) != ("comp_hse", 1):
        rec = g[pre + "dts"][:n]
        tol_dt = 1e-12 if fixture == "comp_heating" else (0.0 if dev.kind == "emu" else TOL_EXACT * n)
        assert np.max(np.abs(np.array(dts) / rec - 1.0)) <= tol_dt
        if n == len(g[pre + "dts"]):
            fin = g[pre + "final"]
            I = (slice(NG, -NG), slice(NG, -NG))
            scale = np.maximum(np.abs(fin[I]).max(axis=(0, 1)), 1e-3)
            tol = 0.0 if dev.kind == "emu" else TOL_EXACT * n
            assert (np.abs(s.download() - fin)[I] / scale).max() <= max(tol, 1e-14 if sponge else 0.0)


# ---- the corner rule ----------------------------------------------------------------------------

def _corners(U):
    return [U[:NG, :NG, 1], U[:NG, -NG:, 1], U[-NG:, :NG, 1], U[-NG:, -NG:, 1]]


@pytest.mark.parametrize("fm", [0, 1])
def test_hse_corner_energy_takes_the_momenta_of_the_previous_fill(dev, golden, fm):
    """outflow / reflecting x sides under hse / hse (c1), momenta stirred: the hse energy of the
    corner blocks comes from the x-ghost density and energy of THIS fill and the x-ghost momenta
    of the PREVIOUS one (fill_BC_all goes variable by variable).  After three steps in the loop
    the four corner blocks are the single steps', bit for bit -- and in this input the other
    candidate (the momenta of this fill: a second fill in a row) is a different number"""
    pre, g, bcs, kw = _case(golden, "comp_hse", 1)
    P, cfl = dev_params(g[pre + "meta"], kernel_set=-1, fast_math=fm, **kw)
    ic = np.nan_to_num(g[pre + "ic"]).copy()
    rng = np.random.default_rng(11)
    ic[NG:-NG, NG:-NG, 2] += 1.e-2 * rng.standard_normal(ic[NG:-NG, NG:-NG, 2].shape)
    ic[NG:-NG, NG:-NG, 3] += 1.e-2 * rng.standard_normal(ic[NG:-NG, NG:-NG, 3].shape)
    f0, mx = g[pre + "drv"]
    ref = _state(dev, g, pre, bcs, ic)
    pref = DtPolicy(BIG, f0, mx)
    dref = _singly(ref, P, cfl, pref, 3)
    Uref = ref.download()
    s = _state(dev, g, pre, bcs, ic)
    pol = DtPolicy(BIG, f0, mx)
    assert [float(x) for x in s.comp_evolve(P, cfl, pol, 3)] == dref
    U = s.download()
    for a, b in zip(_corners(U), _corners(Uref)):
        assert np.array_equal(a, b)
    assert np.array_equal(U, Uref)
    # the two candidates: the next fill (momenta of the fill before) and one more (its own)
    ref.fill_bc()
    A = ref.download()
    ref.fill_bc()
    B = ref.download()
    assert all(not np.array_equal(a, b) for a, b in zip(_corners(A), _corners(B)))
    assert np.array_equal(A[..., (0, 2, 3)], B[..., (0, 2, 3)])


# ---- grid shapes, through the driver ---------------------------------------------------------

def _pyro(dev, monkeypatch, problem, nx, ny, extra=None, solver="compressible", stir=True):
    from pyro2_amd.pyro_sim import Pyro
    monkeypatch.setattr(device.Context, "_default", dev)
    d = {"mesh.nx": nx, "mesh.ny": ny, "driver.max_steps": 1000, "io.do_io": 0, "driver.verbose": 0,
         "vis.dovis": 0}
    d.update(extra or {})
    p = Pyro(solver)
    p.initialize_problem(problem, inputs_dict=d)
    p._quiet = True
    if stir:        # a small velocity perturbation: momenta of both signs everywhere
        cc = p.sim.cc_data
        U = np.array(cc.data)
        rng = np.random.default_rng(5)
        for n in (2, 3):
            U[NG:-NG, NG:-NG, n] += 1.e-3 * U[NG:-NG, NG:-NG, 0] * rng.standard_normal((nx, ny))
        cc.data = U
        del U
    return p


def _snap(p):
    sim = p.sim
    return dict(state=np.array(sim.cc_data.data), t=sim.cc_data.t, n=sim.n, dt=sim.dt, dt_old=sim.dt_old)


def _same(a, b, what=None):
    for key in ("t", "n", "dt", "dt_old"):
        assert a[key] == b[key], (what, key)
    assert np.array_equal(a["state"], b["state"]), what


def _loop_vs_single(dev, monkeypatch, problem, nx, ny, n, extra=None, chunks=None, prep=lambda p: None):
    q = _pyro(dev, monkeypatch, problem, nx, ny, extra)
    prep(q)
    dref = []
    for _ in range(n):
        q.single_step()
        dref.append(float(q.sim.dt))
    p = _pyro(dev, monkeypatch, problem, nx, ny, extra)
    prep(p)
    assert p.sim.can_evolve_many()
    dts = []
    for c in chunks or (n,):
        dts += [float(x) for x in p.sim.evolve_many(c)]
    assert not getattr(p.sim, "_device_stepping_refused", False)
    assert dts == dref
    _same(_snap(p), _snap(q), (problem, nx, ny))
    return p, q


@pytest.mark.parametrize("fm", [0, 1])
@pytest.mark.parametrize("nx,ny", [(300, 8), (8, 300)])
def test_long_thin_grids(dev, monkeypatch, nx, ny, fm):
    """more rows / columns than one workgroup of the fill covers, ragged last pieces, hse / hse"""
    n = 3 if dev.kind == "emu" else 6
    _loop_vs_single(dev, monkeypatch, "hse", nx, ny, n, {"gpu.fast_math": fm}, chunks=(1, n - 1))


@pytest.mark.parametrize("fm", [0, 1])
def test_hse_ambient_sponge_20x36(dev, monkeypatch, fm):
    n = 5 if dev.kind == "emu" else 9
    extra = {"mesh.yrboundary": "ambient", "sponge.do_sponge": 1, "sponge.sponge_rho_begin": 0.5,
             "sponge.sponge_rho_full": 0.1, "sponge.sponge_timescale": 0.01, "gpu.fast_math": fm}

    def ambient(p):         # the state of the top row of the atmosphere, at rest
        cc = p.sim.cc_data
        top = np.array(cc.data)[NG, -NG - 1]
        cc.set_aux("ambient_rho", float(top[0]))
        cc.set_aux("ambient_u", 0.0)
        cc.set_aux("ambient_v", 0.0)
        cc.set_aux("ambient_p", float(top[1] * (cc.get_aux("gamma") - 1.0)))
    p, q = _loop_vs_single(dev, monkeypatch, "hse", 20, 36, n, extra, chunks=(3, n - 3), prep=ambient)
    assert p.sim._params().do_sponge == 1
    U = _snap(p)["state"]
    assert np.all(U[:, -NG:, 0] == p.sim.cc_data.get_aux("ambient_rho"))       # the ambient rows


# ---- the CFL minimum in the hse ghost rows ----------------------------------------------------------

def _cfl_field(U, gamma, dx, dy):
    rho, E, mx, my = (U[..., n] for n in range(4))
    u, v = mx / rho, my / rho
    e = (E - 0.5 * rho * (u * u + v * v)) / rho
    cs = np.sqrt(gamma * (rho * e * (gamma - 1.0)) / rho)
    return np.minimum(dx / (np.abs(u) + cs), dy / (np.abs(v) + cs))


@pytest.mark.parametrize("fm", [0, 1])
def test_cfl_minimum_in_the_hse_ghost_rows(dev, golden, fm):
    """c2 of comp_hse from step 8 on: the CFL limit binds and the whole-array minimum sits in an
    hse ghost row.  The loop's dts are the single steps'; the interior's minimum alone would have
    given another dt"""
    pre, g, bcs, kw = _case(golden, "comp_hse", 2)
    meta = g[pre + "meta"]
    P, cfl = dev_params(meta, kernel_set=-1, fast_math=fm, **kw)
    f0, mx = g[pre + "drv"]
    ref = _state(dev, g, pre, bcs)
    pref = DtPolicy(BIG, f0, mx)
    _singly(ref, P, cfl, pref, 8)
    U8 = ref.download()
    s = _state(dev, g, pre, bcs, U8)
    pol = DtPolicy(BIG, f0, mx)
    pol.t, pol.n, pol.dt_old = pref.t, pref.n, pref.dt_old
    # where the minimum is, on the filled state (a third copy: a fill more would show in the corners)
    probe = _state(dev, g, pre, bcs, U8)
    probe.fill_bc()
    F = _cfl_field(probe.download(), meta[5], meta[3], meta[4])
    i, j = np.unravel_index(np.argmin(F), F.shape)
    assert j < NG or j >= F.shape[1] - NG
    interior = F[NG:-NG, NG:-NG].min()
    assert F.min() < interior
    dt_old8 = pref.dt_old
    dref = _singly(ref, P, cfl, pref, 3)
    assert dref[0] < mx * dt_old8                              # the CFL limit binds, not the growth limit
    assert dref[0] < cfl * interior * (1.0 - 1e-9)
    assert [float(x) for x in s.comp_evolve(P, cfl, pol, 3)] == dref
    assert np.array_equal(s.download(), ref.download())
    _same_policy(pol, pref)


# ---- the sponge ----------------------------------------------------------------------------------

def _sponge_case(golden, fm):
    """the convection set-up (c2 of comp_heating: periodic x, reflecting floor, ambient top, sponge,
    heating) with a fast stream through the thin gas the sponge damps: the velocity maximum -- the
    CFL minimum -- lies where the sponge acts"""
    pre, g, bcs, kw = _case(golden, "comp_heating", 2)
    meta = g[pre + "meta"]
    P, cfl = dev_params(meta, kernel_set=-1, fast_math=fm, **kw)
    ic = np.nan_to_num(g[pre + "ic"]).copy()
    rho = ic[..., 0]
    thin = rho < P.sponge_rho_begin
    thin[:NG], thin[-NG:], thin[:, :NG], thin[:, -NG:] = False, False, False, False
    assert thin.any()
    cs = np.sqrt(meta[5] * _pressure(ic, meta[5]) / rho)
    ic[..., 2] = np.where(thin, 3.0 * cs * rho, ic[..., 2])
    ic[..., 1] += 0.5 * ic[..., 2] ** 2 / rho
    return pre, g, bcs, P, cfl, ic


def _pressure(U, gamma):
    rho, E, mx, my = (U[..., n] for n in range(4))
    return (E - 0.5 * (mx * mx + my * my) / rho) * (gamma - 1.0)


@pytest.mark.parametrize("fm", [0, 1])
def test_policy_sees_the_minimum_behind_the_sponge(dev, golden, fm):
    """every dt is cfl * min (no growth limit): the sponge slows the fastest cells, so the dt after
    a sponge step follows from the partials of the interior BEHIND the sponge -- the step kernel's
    own, from before it, give a smaller one"""
    pre, g, bcs, P, cfl, ic = _sponge_case(golden, fm)
    n = 4
    ref = _state(dev, g, pre, bcs, ic)
    pref = DtPolicy(BIG, 1.0, BIG)
    dref = _singly(ref, P, cfl, pref, n)
    # the same steps without the sponge take other dts from the second one on: it moved the minimum
    Q = device.CompParams.from_buffer_copy(P)
    Q.do_sponge = 0
    nos = _state(dev, g, pre, bcs, ic)
    dnos = _singly(nos, Q, cfl, DtPolicy(BIG, 1.0, BIG), 2)
    assert dnos[0] == dref[0] and dnos[1] < dref[1]
    s = _state(dev, g, pre, bcs, ic)
    pol = DtPolicy(BIG, 1.0, BIG)
    assert [float(x) for x in s.comp_evolve(P, cfl, pol, n)] == dref
    assert np.array_equal(s.download(), ref.download())
    _same_policy(pol, pref)


@pytest.mark.parametrize("fm", [0, 1])
@pytest.mark.parametrize("surplus", [1, 2])
def test_tmax_inside_a_call_with_the_sponge(dev, golden, surplus, fm):
    """the run ends inside the call, an odd and an even number of inactive iterations behind the
    last step: state, ghost frame (the sponge acted on it once per step that advanced, never on an
    inactive iteration), t, n and the cached-minimum state are the single steps'"""
    pre, g, bcs, P, cfl, ic = _sponge_case(golden, fm)
    probe = _state(dev, g, pre, bcs, ic)
    d = _singly(probe, P, cfl, DtPolicy(BIG, 1.0, BIG), 3)
    tmax = d[0] + d[1] + 0.4 * d[2]
    ref = _state(dev, g, pre, bcs, ic)
    pref = DtPolicy(tmax, 1.0, BIG)
    dref = _singly(ref, P, cfl, pref, 10)
    assert len(dref) == 3 and pref.t == tmax
    s = _state(dev, g, pre, bcs, ic)
    pol = DtPolicy(tmax, 1.0, BIG)
    assert [float(x) for x in s.comp_evolve(P, cfl, pol, 3 + surplus)] == dref
    assert np.array_equal(s.download(), ref.download())
    _same_policy(pol, pref)
    assert s.comp_dt_is_cached() == ref.comp_dt_is_cached()
    assert s.comp_dt(P, cfl) == ref.comp_dt(P, cfl)
    assert len(s.comp_evolve(P, cfl, pol, 2)) == 0           # a call on the finished run
    assert np.array_equal(s.download(), ref.download())


# ---- an invalid state ----------------------------------------------------------------------------

@pytest.mark.parametrize("fm", [0, 1])
@pytest.mark.parametrize("at", [0, 2])
def test_invalid_state(dev, golden, at, fm):
    """a negative energy in the interior of the state handed over (the initial one, or the one two
    steps on): ERR_STATE, nothing advances, and the ghost cells are those the hse rules give -- the
    fill a single step makes before its step raises"""
    pre, g, bcs, kw = _case(golden, "comp_hse", 1)
    P, cfl = dev_params(g[pre + "meta"], kernel_set=-1, fast_math=fm, **kw)
    f0, mx = g[pre + "drv"]
    ref = _state(dev, g, pre, bcs)
    pref = DtPolicy(BIG, f0, mx)
    _singly(ref, P, cfl, pref, at)
    U = ref.download()
    U[NG + 3, NG + 5, 1] = -1.0
    ref.upload(U)
    ref.fill_bc()
    ref.comp_dt(P, cfl)
    with pytest.raises(_lib.PyroHipError) as e1:
        ref.comp_step(P, 1.e-6)
    assert e1.value.code == _lib.ERR_STATE
    s = _state(dev, g, pre, bcs, U)
    pol = DtPolicy(BIG, f0, mx)
    pol.t, pol.n, pol.dt_old = pref.t, pref.n, pref.dt_old
    with pytest.raises(_lib.PyroHipError) as e2:
        s.comp_evolve(P, cfl, pol, 3)
    assert e2.value.code == _lib.ERR_STATE and e2.value.steps_done == 0
    assert (pol.t, pol.n) == (pref.t, pref.n)
    got = s.download()
    assert np.array_equal(got, ref.download())
    assert not np.array_equal(got[:, :NG, 1], U[:, :NG, 1])          # the hse rows were filled


# ---- the driver ------------------------------------------------------------------------------------

# (reduced sizes at the cell sizes of the shipped inputs: the trapezoidal atmospheres of bubble and
# convection turn negative on cells several times as tall)
DRIVER = [("rt", 16, 48, {}),
          ("bubble", 16, 32, {"mesh.xmax": 0.5, "mesh.ymax": 1.0, "bubble.x_pert": 0.25, "bubble.y_pert": 0.3,
                              "bubble.r_pert": 0.12}),
          ("convection", 16, 48, {})]


@pytest.mark.parametrize("fm", [0, 1])
@pytest.mark.parametrize("problem,nx,ny,extra", DRIVER)
def test_run_sim_steps_on_the_device(dev, monkeypatch, problem, nx, ny, extra, fm):
    n = 4 if dev.kind == "emu" else 12
    extra = dict(extra, **{"driver.max_steps": n, "gpu.fast_math": fm})
    q = _pyro(dev, monkeypatch, problem, nx, ny, extra, stir=False)
    monkeypatch.setattr(q.sim, "can_evolve_many", lambda: False)
    q.run_sim()
    p = _pyro(dev, monkeypatch, problem, nx, ny, extra, stir=False)
    assert p.sim.can_evolve_many() is True
    calls, steps = [], []
    many, single = p.sim.evolve_many, type(p).single_step
    monkeypatch.setattr(p.sim, "evolve_many", lambda k: (calls.append(k), many(k))[1])
    monkeypatch.setattr(type(p), "single_step", lambda self: (steps.append(1), single(self))[1])
    p.run_sim()
    assert p.sim.n == n and sum(calls) >= n and not steps
    assert not getattr(p.sim, "_device_stepping_refused", False)
    _same(_snap(p), _snap(q), problem)
    if problem == "convection":
        assert p.sim._params().do_sponge == 1 and p.sim._heating() is not None


def test_refusals(dev, monkeypatch):
    """what keeps stepping singly: the ramp boundary, a stratified run on slabs, compressible_rk
    with the sponge, tracer particles under hse sides"""
    ramp = _pyro(dev, monkeypatch, "ramp", 32, 8, stir=False)
    assert ramp.sim.can_evolve_many() is False
    rk = _pyro(dev, monkeypatch, "hse", 16, 48, {"sponge.do_sponge": 1}, solver="compressible_rk", stir=False)
    assert rk.sim.can_evolve_many() is False
    tracers = _pyro(dev, monkeypatch, "hse", 16, 48, {"particles.do_particles": 1, "particles.n_particles": 16},
                    stir=False)
    assert tracers.sim.particles is not None and tracers.sim.can_evolve_many() is False
    plain = _pyro(dev, monkeypatch, "hse", 16, 48, stir=False)
    assert plain.sim.can_evolve_many() is True
    # the same run as one slab of two (no transport: nothing may be sent)
    monkeypatch.setattr(plain.sim.cc_data, "slab", object())
    assert plain.sim.can_evolve_many() is False


def test_library_refusals_keep_their_wording(dev, golden):
    """what pyrohip_comp_evolve still refuses says "device-side stepping:" (the driver's fallback
    reads that): user boundaries or the sponge with a tracer set bound; and a state whose hse
    parameters were never set is an argument error"""
    pre, g, bcs, kw = _case(golden, "comp_hse", 0)
    P, cfl = dev_params(g[pre + "meta"], kernel_set=-1, **kw)
    meta = g[pre + "meta"]
    s = comp_state(dev, int(meta[0]), int(meta[1]), bcs)
    s.upload(np.nan_to_num(g[pre + "ic"]))
    with pytest.raises(_lib.PyroHipError, match="pyrohip_state_set_user_bc"):
        s.comp_evolve(P, cfl, DtPolicy(BIG), 2)
    P0 = device.CompParams.from_buffer_copy(P)
    P0.kernel_set = 0
    s.set_user_bc(meta[5], meta[12], meta[4], g[pre + "ambient"])
    with pytest.raises(_lib.PyroHipError, match="kernel_set 0"):
        s.comp_evolve(P0, cfl, DtPolicy(BIG), 2)


# ---- the row-marching kernel ---------------------------------------------------------------------

@pytest.mark.gpu
def test_row_marching_kernel_under_hse(hip, monkeypatch):
    """the smallest grid the contracted build steps with k_ctu_wave (1024 x 1024), hse / hse"""
    hip.kind = "hip"
    _loop_vs_single(hip, monkeypatch, "hse", 1024, 1024, 6, {"gpu.fast_math": 1}, chunks=(3, 3))


# ---- plain states: the same launches as before ---------------------------------------------------

def test_plain_state_launches_unchanged(dev, golden):
    """Sedov 64^2, five steps in the loop: the kernels launched are those of the loop without
    hse / ambient sides and without the sponge -- the one-launch fill and the sponge kernel never
    appear -- and the result is the single steps'"""
    from test_device_compressible import device_comp_run
    g = golden("comp_sedov_64_020")
    meta = g["meta"]
    ic = np.nan_to_num(g["ic"])
    bcs = ["outflow"] * 4
    Uref, dref, _ = device_comp_run(dev, ic, meta, bcs, 0.1, 5, kernel_set=-1)
    P, cfl = dev_params(meta, kernel_set=-1)
    s = comp_state(dev, 64, 64, bcs)
    s.upload(ic)
    dev.prof_enable(True)
    try:
        dev.prof_report()
        dts = s.comp_evolve(P, cfl, DtPolicy(0.1), 5)
        launches = {name: n for name, (n, _) in dev.prof_report().items()}
    finally:
        dev.prof_enable(False)
    assert list(dts) == list(dref) and np.array_equal(s.download(), Uref)
    # (the launches the library times: the policy before every step and the closing one, the tile
    # kernel, which applies the boundary rules itself from the second step on)
    assert launches == {"k_dt_policy": 6, "k_ctu_fused": 5}
