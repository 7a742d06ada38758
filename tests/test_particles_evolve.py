"""Tracer particles inside the device-side stepping loops (DESIGN.md 15.1:
pyrohip_comp_evolve_p / pyrohip_comp_rk_evolve_p / pyrohip_swe_evolve_p, the
run-protocol forms of the three particle launches in csrc/particles.hip).

One evolve_many(n) that carries the set through the run is held to n x
Pyro.single_step with gpu.device_particles = 1 -- the path that
tests/test_particles_device.py pins to the reference: state, positions, initial
positions, velocities, ORDER, live count, t, n, dt, dt_old and the dt sequence.
Every comparison is np.array_equal."""
import types

import numpy as np
import pytest

from helpers import DtPolicy
from pyro2_amd import _lib, device
from pyro2_amd.particles import particles
from test_device_compressible import comp_state, dev_params

ERR_ARG = 10001                         # PYROHIP_ERR_ARG (include/pyrohip.h)
N_ODD, N_EVEN = 7, 12                   # odd and even buffer parity of the state and of the set

LEGS = {
    "ctu": ("compressible", "sedov", None, {"sedov.r_init": 0.15}),
    "rk4": ("compressible_rk", "sedov", None, {"sedov.r_init": 0.15, "gpu.kernel_set": 2,
                                               "compressible.temporal_method": "RK4"}),
    "tvd2": ("compressible_rk", "sedov", None, {"sedov.r_init": 0.15, "gpu.kernel_set": 2,
                                                "compressible.temporal_method": "TVD2"}),
    "swe": ("swe", "dam", "inputs.dam.x", {"mesh.ymax": 1.0}),
}


def _pyro(dev, monkeypatch, leg, nx=32, ny=32, extra=None, pos=None, npart=100):
    """an initialised Pyro of LEGS[leg] on `dev`; pos: an (n, 2) array that replaces the grid of
    npart tracers (the "array" generator)"""
    from pyro2_amd.pyro_sim import Pyro
    monkeypatch.setattr(device.Context, "_default", dev)
    solver, problem, inputs, over = LEGS[leg] if isinstance(leg, str) else leg
    d = {"mesh.nx": nx, "mesh.ny": ny, "driver.max_steps": 1000, "io.do_io": 0, "driver.verbose": 0,
         "particles.do_particles": 1, "particles.n_particles": npart,
         "particles.particle_generator": "grid", "gpu.device_particles": 1}
    d.update(over)
    d.update(extra or {})
    p = Pyro(solver)
    p.initialize_problem(problem, inputs_file=inputs, inputs_dict=d)
    if pos is not None:
        old = p.sim.particles
        p.sim.particles = particles.Particles(old.sim_data, old.bc, len(pos), "array", np.array(pos, dtype=np.float64))
    return p


def _snap(p):
    """everything the issue compares, as host arrays (this downloads: only at the end of a run)"""
    sim, ps = p.sim, p.sim.particles
    return dict(state=np.array(sim.cc_data.data), pos=np.array(ps.get_positions()),
                init=np.array(ps.get_init_positions()), vel=np.array(ps.vel), count=ps.n_particles,
                t=sim.cc_data.t, n=sim.n, dt=getattr(sim, "dt", None), dt_old=getattr(sim, "dt_old", None))


def _same(a, b, what=None, skip=()):
    for k in a:
        if k in skip:
            continue
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def _single(p, nsteps):
    """nsteps x Pyro.single_step (fewer if the run finishes); -> the time steps"""
    dts = []
    for _ in range(nsteps):
        if p.sim.finished():
            break
        p.single_step()
        dts.append(float(p.sim.dt))
    return dts


class _NoDownloads:
    """DeviceState.download / download_var / download_rows are not called while armed"""

    def __init__(self, monkeypatch):
        self.n = 0
        for name in ("download", "download_var", "download_rows"):
            monkeypatch.setattr(device.DeviceState, name, self._wrap(getattr(device.DeviceState, name)))

    def _wrap(self, f):
        def g(*a, **k):
            self.n += 1
            return f(*a, **k)
        return g


def _many(p, nsteps, monkeypatch):
    """one evolve_many(nsteps) that must take the device loop and never download the state"""
    assert p.sim.can_evolve_many()
    counter = _NoDownloads(monkeypatch)
    dts = [float(x) for x in p.sim.evolve_many(nsteps)]
    assert counter.n == 0
    assert not p.sim.particles._host_valid or p.sim.particles.n_particles == 0   # the set stayed on the device
    return dts


# ---- 1. parity with single steps --------------------------------------------------------
_REF = {}


def _reference(dev, monkeypatch, leg, nx, ny, fm, n, pos_key=None, pos=None):
    """(dts, snapshot) of n single steps, once per case.  (One run per n: a look at the state in
    the middle of a run downloads it, and the next step then takes its CFL minimum afresh instead
    of from the step kernel -- another single-step run than the one evolve_many stands for.)"""
    key = (dev.kind, leg, nx, ny, fm, n, pos_key)
    if key not in _REF:
        p = _pyro(dev, monkeypatch, leg, nx, ny, {"gpu.fast_math": fm}, pos=pos)
        dts = _single(p, n)
        assert len(dts) == n
        _REF[key] = (dts, _snap(p))
    return _REF[key]


@pytest.mark.parametrize("n", [N_ODD, N_EVEN])
@pytest.mark.parametrize("fm", [0, 1])
@pytest.mark.parametrize("nx,ny", [(32, 32), (24, 40)])
@pytest.mark.parametrize("leg", list(LEGS))
def test_parity_with_single_steps(dev, monkeypatch, leg, nx, ny, fm, n):
    dts, ref = _reference(dev, monkeypatch, leg, nx, ny, fm, n)
    p = _pyro(dev, monkeypatch, leg, nx, ny, {"gpu.fast_math": fm})
    got = _many(p, n, monkeypatch)
    assert got == dts
    _same(_snap(p), ref, (leg, nx, ny, fm, n))
    assert 0 < ref["count"] <= 100 and np.any(ref["pos"] != ref["init"])   # the tracers did move


@pytest.mark.parametrize("count", [1, 255, 256, 257, 513])
def test_parity_at_the_workgroup_edges_of_the_scans(dev, monkeypatch, count):
    rng = np.random.default_rng(100 + count)
    pos = rng.uniform(0.02, 0.98, (count, 2))
    for n in (N_ODD, N_EVEN):
        dts, ref = _reference(dev, monkeypatch, "ctu", 32, 32, 0, n, pos_key=count, pos=pos)
        p = _pyro(dev, monkeypatch, "ctu", 32, 32, {"gpu.fast_math": 0}, pos=pos)
        assert _many(p, n, monkeypatch) == dts
        _same(_snap(p), ref, (count, n))
        assert ref["count"] == count


# ---- 2. it actually took the device loop ------------------------------------------------
@pytest.mark.parametrize("leg", list(LEGS))
def test_particles_do_not_leave_the_device_loop(dev, monkeypatch, leg):
    p = _pyro(dev, monkeypatch, leg)
    assert p.sim.particles is not None
    assert p.sim.can_evolve_many() is True


def test_run_sim_with_particles_reaches_evolve_many(dev, monkeypatch):
    p = _pyro(dev, monkeypatch, "ctu", extra={"driver.max_steps": N_ODD})
    calls, steps = [], []
    many, single = p.sim.evolve_many, type(p).single_step
    monkeypatch.setattr(p.sim, "evolve_many", lambda k: (calls.append(k), many(k))[1])
    monkeypatch.setattr(type(p), "single_step", lambda self: (steps.append(1), single(self))[1])
    p.run_sim()
    assert p.sim.n == N_ODD and sum(calls) >= N_ODD and not steps
    dts, ref = _reference(dev, monkeypatch, "ctu", 32, 32, 1, N_ODD)     # (gpu.fast_math defaults to 1)
    _same(_snap(p), ref, "run_sim")


# ---- 3. upper-border ghost cells --------------------------------------------------------
def _border_positions(g, frac=0.3):
    """less than half a cell inside each upper border and each corner (their 2 x 2 stencils take
    ghost row ilo + nx / ghost column jlo + ny), and one in the middle"""
    xm, ym = 0.5 * (g.xmin + g.xmax) + 0.01, 0.5 * (g.ymin + g.ymax) - 0.02
    xl, xh = g.xmin + frac * g.dx, g.xmax - frac * g.dx
    yl, yh = g.ymin + frac * g.dy, g.ymax - frac * g.dy
    return np.array([[xh, ym], [xm, yh], [xh, yh], [xh, yl], [xl, yh], [xl, yl], [xl, ym], [xm, yl], [xm, ym],
                     [g.xmax - 0.05 * g.dx, ym], [xm, g.ymax - 0.05 * g.dy], [g.xmax - 0.45 * g.dx, g.ymax - 0.45 * g.dy]])


ADVECT = ("compressible", "advect", None, {})
WALLS = {"mesh.xlboundary": "reflect", "mesh.xrboundary": "reflect",
         "mesh.ylboundary": "reflect", "mesh.yrboundary": "reflect"}


@pytest.mark.parametrize("n", [5, 6])
@pytest.mark.parametrize("walls", [False, True])
@pytest.mark.parametrize("solver", ["compressible", "compressible_rk", "swe"])
def test_upper_border_ghost_cells(dev, monkeypatch, solver, walls, n):
    """a periodic problem (advect: u = v = 1 carries the tracers across the upper borders) and the
    same flow between reflecting walls (the momenta change sign across them); swe: the dam, which
    has outflow sides in x, and the dam between walls"""
    if solver == "swe":
        leg, extra = LEGS["swe"], (WALLS if walls else {})
    else:
        leg = (solver, "advect", None, {"gpu.kernel_set": 2} if solver == "compressible_rk" else {})
        extra = WALLS if walls else {}
    nx, ny = 24, 40

    def make():
        p = _pyro(dev, monkeypatch, leg, nx, ny, extra, npart=1)
        pos = _border_positions(p.sim.cc_data.grid)
        old = p.sim.particles
        p.sim.particles = particles.Particles(old.sim_data, old.bc, len(pos), "array", pos)
        return p

    a = make()
    dts = _single(a, n)
    b = make()
    assert _many(b, n, monkeypatch) == dts
    ref = _snap(a)
    _same(_snap(b), ref, (solver, walls, n))
    assert np.any(ref["vel"] != 0.0) and np.any(ref["pos"] != ref["init"])


def _bare_advect(nx, ny, ng, bcs):
    """the advect problem's state on a unit square, boundary fill left to the device"""
    x = (np.arange(nx + 2 * ng) - ng + 0.5) / nx
    y = (np.arange(ny + 2 * ng) - ng + 0.5) / ny
    X, Y = np.meshgrid(x, y, indexing="ij")
    U = np.zeros((nx + 2 * ng, ny + 2 * ng, 4))
    U[..., 0] = 1.0 + np.exp(-60.0 * ((X - 0.5) ** 2 + (Y - 0.5) ** 2))
    U[..., 2] = U[..., 0] * 1.0
    U[..., 3] = U[..., 0] * 0.7
    U[..., 1] = 1.0 / 0.4 + 0.5 * (U[..., 2] ** 2 + U[..., 3] ** 2) / U[..., 0]
    return U


class _Bare:
    """compressible at the bare entry points: a state, a particle set, and the two ways to run"""
    RATIO = ("ratio", (2, 3, 0))

    def __init__(self, dev, nx, ny, bcs, U0, pos, cfl=0.8, pbc=None, f0=0.5, **kw):
        ng = 4
        self.meta = [nx, ny, ng, 1.0 / nx, 1.0 / ny, 1.4, 2, 1, 0.75, 0.85, 0.33, 0.1, 0.0, cfl]
        self.P, self.cfl = dev_params(self.meta, **kw)
        self.s = comp_state(dev, nx, ny, bcs)
        self.s.upload(U0)
        self.grid = types.SimpleNamespace(xmin=0.0, xmax=1.0, ymin=0.0, ymax=1.0, dx=1.0 / nx, dy=1.0 / ny)
        self.pbc = pbc or ["reflect-even" if b == "reflect" else b for b in bcs]
        self.dp = device.DeviceParticles(dev, pos)
        self.pol = DtPolicy(1.e30, init_tstep_factor=f0)

    def single(self, nsteps):
        """-> (dts, error or None): fill, dt policy, step, particle advance, one by one"""
        dts = []
        for _ in range(nsteps):
            try:
                self.s.fill_bc()
                dt = self.pol(self.s.comp_dt(self.P, self.cfl))
                self.s.comp_step(self.P, dt)
                self.dp.advance(self.s, self.grid, self.pbc, *self.RATIO, dt)
            except _lib.PyroHipError as e:
                return dts, e
            self.pol.advance(dt)
            dts.append(dt)
        return dts, None

    def many(self, nsteps):
        bound = (self.dp, self.dp.params(self.grid, self.pbc, *self.RATIO))
        try:
            return list(self.s.comp_evolve(self.P, self.cfl, self.pol, nsteps, particles=bound)), None
        except _lib.PyroHipError as e:
            return list(e.dts), e

    def snap(self, ghosts=True):
        pos, init, vel = self.dp.download()
        U = self.s.download()
        return dict(state=U if ghosts else U[4:-4, 4:-4], pos=pos, init=init, vel=vel, count=self.dp.count(),
                    t=self.pol.t, n=self.pol.n, dt_old=self.pol.dt_old)


# kernel_set 1: the tile kernel; 2: the row-marching kernel with its evolve modes -- the library's
# choice, one launch per step (falls back to three with a set bound: the one-launch steps write no
# ghost cell) and three launches per step
MODES = [dict(kernel_set=1), dict(kernel_set=2, march_rows=11, step_launches=0),
         dict(kernel_set=2, march_rows=11, step_launches=1), dict(kernel_set=2, march_rows=11, step_launches=3)]


@pytest.mark.parametrize("bcs", [["periodic"] * 4, ["reflect"] * 4], ids=["periodic", "walls"])
@pytest.mark.parametrize("mode", range(len(MODES)))
def test_upper_border_ghost_cells_in_every_evolve_mode(dev, mode, bcs):
    nx, ny = 24, 40
    U0 = _bare_advect(nx, ny, 4, bcs)
    pos = _border_positions(types.SimpleNamespace(xmin=0.0, xmax=1.0, ymin=0.0, ymax=1.0, dx=1.0 / nx, dy=1.0 / ny))
    for n in (5, 6):
        a = _Bare(dev, nx, ny, bcs, U0, pos, **MODES[mode])
        b = _Bare(dev, nx, ny, bcs, U0, pos, **MODES[mode])
        dts, err = a.single(n)
        assert err is None
        got, err = b.many(n)
        assert err is None and got == dts
        _same(b.snap(), a.snap(), (mode, n))


# ---- 4. dropping ------------------------------------------------------------------------
OUTFLOW = {"mesh.xlboundary": "outflow", "mesh.xrboundary": "outflow",
           "mesh.ylboundary": "outflow", "mesh.yrboundary": "outflow"}


def _drop_run(dev, monkeypatch, pos_of, n):
    def make():
        p = _pyro(dev, monkeypatch, ADVECT, 32, 32, OUTFLOW, npart=1)
        old = p.sim.particles
        pos = pos_of(p.sim.cc_data.grid)
        p.sim.particles = particles.Particles(old.sim_data, old.bc, len(pos), "array", pos)
        return p, len(pos)
    a, n0 = make()
    counts = []
    for _ in range(n):
        a.single_step()
        counts.append(a.sim.particles.n_particles)
    b, _ = make()
    dts = _many(b, n, monkeypatch)
    assert len(dts) == n
    return n0, counts, _snap(a), _snap(b)


def test_dropping_in_several_steps(dev, monkeypatch):
    """the advect state with outflow on every side: u = v = 1 carries tracers out through the upper
    borders, a few per step"""
    def pos_of(g):
        # a diagonal ladder below the upper-right corner, rungs a fifth of a cell apart, and
        # a block in the middle that stays
        k = np.arange(40)
        near = np.stack([g.xmax - (0.02 + 0.2 * k) * g.dx, g.ymax - (0.5 + 0.21 * k) * g.dy], axis=1)
        mid = np.stack([0.3 + 0.01 * np.arange(30), 0.4 + 0.005 * np.arange(30)], axis=1)
        return np.concatenate([near, mid])
    n0, counts, ref, got = _drop_run(dev, monkeypatch, pos_of, N_EVEN)
    # (conditions on the input, established on the single-step run)
    assert 0 < counts[-1] < n0
    assert len(set(counts)) >= 4                 # the count shrank in several different steps
    _same(got, ref, "dropping")


def test_the_set_empties_mid_run_and_the_run_carries_on(dev, monkeypatch):
    def pos_of(g):
        k = np.arange(20)
        return np.stack([g.xmax - (0.01 + 0.01 * k) * g.dx, 0.2 + 0.03 * k], axis=1)
    n0, counts, ref, got = _drop_run(dev, monkeypatch, pos_of, N_ODD)
    assert counts[-1] == 0 and counts[0] > 0 and counts.index(0) < N_ODD - 1
    _same(got, ref, "emptied")
    assert got["n"] == N_ODD and got["pos"].shape == (0, 2)


# ---- 5. inactive iterations -------------------------------------------------------------
@pytest.mark.parametrize("surplus", [3, 4])
@pytest.mark.parametrize("leg", ["ctu", "rk4", "swe"])
def test_inactive_iterations_leave_the_set_alone(dev, monkeypatch, leg, surplus):
    """max_steps beyond the steps to tmax by an odd and an even surplus: the order and the buffers
    are those of the single-step run that stopped at tmax, and a second call changes nothing"""
    a = _pyro(dev, monkeypatch, leg)
    dts = _single(a, 4)
    tmax = sum(dts) + 0.4 * dts[-1]                    # ends inside the fifth step
    a = _pyro(dev, monkeypatch, leg, extra={"driver.tmax": tmax})
    dts = _single(a, 50)
    nsteps = len(dts)
    assert a.sim.finished() and nsteps == 5
    b = _pyro(dev, monkeypatch, leg, extra={"driver.tmax": tmax})
    assert _many(b, nsteps + surplus, monkeypatch) == dts
    ref = _snap(a)
    _same(_snap(b), ref, (leg, surplus))
    assert b.sim.cc_data.t == tmax
    # the finished run, once more
    assert list(b.sim.evolve_many(surplus)) == []
    _same(_snap(b), ref, (leg, surplus, "again"), skip=("state",))
    assert np.array_equal(np.array(b.sim.cc_data.data)[4:-4, 4:-4], ref["state"][4:-4, 4:-4])


# ---- 6. invalid state -------------------------------------------------------------------
def _unstable_state(nx, ny, ng=4):
    x = (np.arange(nx + 2 * ng) - ng + 0.5) / nx
    y = (np.arange(ny + 2 * ng) - ng + 0.5) / ny
    X, Y = np.meshgrid(x, y, indexing="ij")
    rho = 1.0 + 0.2 * np.sin(2 * np.pi * X) * np.cos(2 * np.pi * Y)
    u, v = 0.5 + 0.3 * np.sin(2 * np.pi * Y), -0.4 + 0.3 * np.cos(2 * np.pi * X)
    p = 1.0 + 5.0 * np.exp(-80 * ((X - 0.5) ** 2 + (Y - 0.5) ** 2))
    U = np.zeros((nx + 2 * ng, ny + 2 * ng, 4))
    U[..., 0], U[..., 2], U[..., 3] = rho, rho * u, rho * v
    U[..., 1] = p / 0.4 + 0.5 * rho * (u * u + v * v)
    return U


@pytest.mark.parametrize("kw", [dict(kernel_set=1), dict(kernel_set=2, march_rows=11)], ids=["tile", "wave"])
def test_invalid_state_at_the_first_step_leaves_the_set_untouched(dev, kw):
    nx, ny = 20, 28
    U0 = _unstable_state(nx, ny)
    U0[4 + 7, 4 + 9, 1] = -1.0                         # a negative energy: invalid as handed over
    pos = np.random.default_rng(5).uniform(0.05, 0.95, (300, 2))
    b = _Bare(dev, nx, ny, ["periodic"] * 4, U0, pos, **kw)
    before = b.snap(ghosts=False)
    dts, err = b.many(4)
    assert err is not None and err.code == _lib.ERR_STATE and err.steps_done == 0 and dts == []
    assert "particle" not in str(err)
    # positions, order, velocities, count, t, n (dt_old is the policy's, set before the step: as without a set)
    _same(b.snap(ghosts=False), before, "first step", skip=("dt_old",))


@pytest.mark.parametrize("surplus", [2, 3])
@pytest.mark.parametrize("kw", [dict(kernel_set=1), dict(kernel_set=2, march_rows=11)], ids=["tile", "wave"])
def test_invalid_state_after_k_steps(dev, kw, surplus):
    """a CFL number of 2 lets the run go unstable after a few steps (the very same steps on both
    paths): the set is the single-step set after the k steps that advanced"""
    nx, ny = 20, 28
    U0 = _unstable_state(nx, ny)
    pos = np.random.default_rng(6).uniform(0.05, 0.95, (300, 2))
    a = _Bare(dev, nx, ny, ["periodic"] * 4, U0, pos, cfl=2.0, **kw)
    dts, err = a.single(30)
    k = len(dts)
    assert err is not None and err.code == _lib.ERR_STATE and 0 < k < 30      # (a condition on the input)
    b = _Bare(dev, nx, ny, ["periodic"] * 4, U0, pos, cfl=2.0, **kw)
    got, err = b.many(k + surplus)
    assert err is not None and err.code == _lib.ERR_STATE and err.steps_done == k and got == dts
    assert "particle" not in str(err)
    _same(b.snap(ghosts=False), a.snap(ghosts=False), ("after", k))


# ---- 7. particle error ------------------------------------------------------------------
OFF = 2


def test_particle_error_ends_the_run(dev, monkeypatch):
    """swe with a NaN momentum planted in one cell, OFF cells from a tracer: the first step carries
    the NaN as far as its stencil reaches, short of the tracer; the second one brings it under the
    tracer, whose midpoint position is then NaN: nothing to interpolate at"""
    def make():
        p = _pyro(dev, monkeypatch, "swe", npart=1)
        cc = p.sim.cc_data
        g = cc.grid
        i, j = 20, 11
        cc.get_var("x-momentum")[g.ilo + i, g.jlo + j] = np.nan
        old = p.sim.particles
        pos = np.array([[0.31, 0.52], [g.xmin + (i + OFF + 0.6) * g.dx, g.ymin + (j + 0.7) * g.dy], [0.7, 0.2]])
        p.sim.particles = particles.Particles(old.sim_data, old.bc, len(pos), "array", pos)
        return p
    a = make()
    a.single_step()
    with pytest.raises(_lib.PyroHipError) as e:
        a.single_step()
    assert e.value.code == _lib.ERR_STATE and a.sim.n == 1
    ref = _snap(a)
    # the state after n = 1 steps (the single-step path has advanced it once more)
    c = make()
    c.single_step()
    state1 = np.array(c.sim.cc_data.data)
    b = make()
    assert b.sim.can_evolve_many()
    with pytest.raises(_lib.PyroHipError) as e:
        b.sim.evolve_many(5)
    assert e.value.code == _lib.ERR_STATE and "particle" in str(e.value) and e.value.steps_done == 1
    got = _snap(b)
    _same(got, ref, "particle error", skip=("state", "dt"))
    assert np.array_equal(got["state"][4:-4, 4:-4], state1[4:-4, 4:-4], equal_nan=True)


def test_a_set_on_a_slab_is_an_argument_error(dev):
    nx, ny = 20, 28
    b = _Bare(dev, nx, ny, ["periodic"] * 4, _unstable_state(nx, ny), np.full((3, 2), 0.5), kernel_set=1)
    b.s.set_neighbours(1, -1)
    before = b.snap()
    dts, err = b.many(2)
    assert err is not None and err.code == ERR_ARG and "particles" in str(err)
    _same(b.snap(), before, "refused")


# ---- 8. nothing else moved --------------------------------------------------------------
@pytest.mark.parametrize("leg", list(LEGS))
def test_a_set_on_the_host_path_still_steps_singly(dev, monkeypatch, leg):
    p = _pyro(dev, monkeypatch, leg, extra={"gpu.device_particles": 0})
    assert p.sim.particles is not None and p.sim.can_evolve_many() is False


@pytest.mark.parametrize("leg", ["compressible_fv4", "compressible_sdc"])
def test_fourth_order_solvers_keep_stepping_singly(dev, monkeypatch, leg):
    p = _pyro(dev, monkeypatch, (leg, "sedov", None, {"sedov.r_init": 0.15}))
    assert p.sim.can_evolve_many() is False


@pytest.mark.parametrize("leg", ["ctu", "rk4", "swe"])
def test_nothing_bound_runs_as_before(dev, monkeypatch, leg):
    """without particles the three entry points give what single steps give"""
    off = {"particles.do_particles": 0}
    a = _pyro(dev, monkeypatch, leg, extra=off)
    assert a.sim.particles is None
    dts = []
    for _ in range(N_ODD):
        a.single_step()
        dts.append(float(a.sim.dt))
    b = _pyro(dev, monkeypatch, leg, extra=off)
    assert b.sim.can_evolve_many()
    assert [float(x) for x in b.sim.evolve_many(N_ODD)] == dts
    assert np.array_equal(np.array(b.sim.cc_data.data), np.array(a.sim.cc_data.data))
    assert (b.sim.cc_data.t, b.sim.n, b.sim.dt_old) == (a.sim.cc_data.t, a.sim.n, a.sim.dt_old)
