"""advection_rk and advection_fv4 (method-of-lines advection of a scalar with a constant velocity,
second and fourth order) on the device against runs of the reference (tools/gen_advrk_golden.py):
the stage kernel of csrc/advection_rk.hip stage by stage, the fused Runge-Kutta step against the
stage-by-stage path, the several-steps call, short runs through the driver, the reference's two
regression problems and their stored output files, the output files this package writes, tracer
particles and the refusals.

Tolerances.  The bit-faithful build (gpu.fast_math = 0: no FMA contraction, the reference's
operation order, true divisions by dx and dy) is held to equality, ghost frame included.  The
contracted build is held to the project's advection tolerance, 1e-12 by conftest.max_rel_err, for
one step (the reference's own step moves by less than 1e-15 under 1e-15 relative noise on its
input in every recorded case: `twin_dev` of advrk_stages.npz, asserted <= 1e-12 by the generator);
for the 81 steps of the regression runs to max(10 x twin_dev, 1e-12), twin_dev being what a run of
the reference with 1e-15 relative noise on its initial data differs by from the clean one
(advrk_regress.npz; measured figures: DESIGN)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, max_rel_err
from pyro2_amd import _lib, device
from pyro2_amd.mesh import integration

NCASES = 14
SOLVER = {2: "advection_rk", 4: "advection_fv4"}
STORED = {2: "advrk_smooth_0081.h5", 4: "advfv4_smooth_0081.h5"}
GRIDS = ((33, 36), (16, 19))
ERR_ARG = 10001


def _case(golden, k):
    g = golden("advrk_stages")
    assert int(g["ncases"]) == NCASES
    pre = f"c{k}_"
    m = g[pre + "meta"]
    c = {"nx": int(m[0]), "ny": int(m[1]), "ng": int(m[2]), "lim": int(m[3]), "scheme": int(m[4]),
         "dx": float(m[5]), "dy": float(m[6]), "u": float(m[7]), "v": float(m[8]), "cfl": float(m[9]),
         "ns": int(m[10]), "method": str(g[pre + "method"]), "bc": [str(b) for b in g[pre + "bc"]],
         "Uin": g[pre + "Uin"], "new": g[pre + "new"], "dt": float(g[pre + "dt"]),
         "twin_dev": float(g[pre + "twin_dev"])}
    c["stages"] = [{key: g[f"{pre}s{s}_{key}"] for key in ("start", "a_x", "a_y", "F_x", "F_y", "k")}
                   for s in range(c["ns"])]
    return c


def _state(dev, c, bc=None, ng=None):
    s = device.DeviceState(dev, c["nx"], c["ny"], c["ng"] if ng is None else ng, [bc or c["bc"]])
    if ng is None:
        s.upload(np.ascontiguousarray(c["Uin"][:, :, None]))
    return s


def _plane(s):
    return np.ascontiguousarray(s.download()[:, :, 0])


def _params(c, fast_math=0, **over):
    kw = dict(dx=c["dx"], dy=c["dy"], u=c["u"], v=c["v"], limiter=c["lim"], scheme=c["scheme"])
    kw.update(over)
    return _lib.AdvRkParams(kw["dx"], kw["dy"], kw["u"], kw["v"], kw["limiter"], kw["scheme"], fast_math)


def _same(got, ref, what):
    d = np.abs(np.asarray(got) - np.asarray(ref)).max()
    print(f"{what}: max |diff| = {d:.3e}, max |ref| = {np.abs(ref).max():.3e}")
    assert np.array_equal(got, ref), (what, d)


def test_cases_cover_the_issue(golden):
    """the recorded cases: both schemes, every limiter, every method, the three boundary kinds,
    zero and negative velocity components, grids smaller than a tile and of several ragged tiles"""
    cs = [_case(golden, k) for k in range(NCASES)]
    assert {(c["scheme"], c["lim"]) for c in cs} == {(2, 0), (2, 1), (2, 2), (4, 0), (4, 1)}
    assert {c["method"] for c in cs} == {"RK2", "TVD2", "TVD3", "RK4"}
    assert {b for c in cs for b in c["bc"]} == {"periodic", "outflow", "reflect-even"}
    assert {(c["nx"], c["ny"]) for c in cs} >= {(33, 36), (16, 19), (4, 5), (8, 8)}
    assert {(c["u"], c["v"]) for c in cs} >= {(1.0, 1.0), (-1.0, 0.5), (0.7, -1.0), (0.0, 1.0), (-1.0, 0.0)}
    assert any(c["scheme"] == 4 and c["dx"] != c["dy"] for c in cs)
    assert all(c["twin_dev"] <= 1e-12 for c in cs)


@pytest.mark.parametrize("k", range(NCASES))
def test_stages_bit_for_bit(dev, golden, k):
    """one evolve() of the reference per case, from a plane whose ghost cells hold junk (every
    stage applies the boundary rules itself).  Per stage the stage start with its ghost cells,
    the face values and fluxes where the update reads them and k_s, then the new density with its
    ghost frame: equal to the reference's, bit for bit."""
    c = _case(golden, k)
    ng, nx, ny = c["ng"], c["nx"], c["ny"]
    s = _state(dev, c)
    P = _params(c)
    t = 1 if c["scheme"] == 4 else 0      # the fourth-order fluxes read face averages one face sideways
    ax = (slice(ng, ng + nx + 1), slice(ng - t, ng + ny + t))
    ay = (slice(ng - t, ng + nx + t), slice(ng, ng + ny + 1))
    fx = (slice(ng, ng + nx + 1), slice(ng, ng + ny))
    fy = (slice(ng, ng + nx), slice(ng, ng + ny + 1))
    inner = (slice(ng, ng + nx), slice(ng, ng + ny))
    for n, ref in enumerate(c["stages"]):
        st = s.advrk_stages(0, P, c["method"], c["dt"], n)
        _same(st[5], ref["start"], f"stage {n}: stage start, ghost cells included")
        _same(st[0][ax], ref["a_x"][ax], f"stage {n}: a_x")
        _same(st[1][ay], ref["a_y"][ay], f"stage {n}: a_y")
        _same(st[2][fx], ref["F_x"][fx], f"stage {n}: F_x")
        _same(st[3][fy], ref["F_y"][fy], f"stage {n}: F_y")
        _same(st[4][inner], ref["k"][inner], f"stage {n}: k")
        assert np.abs(ref["k"][inner]).max() > 0.0
    _same(_plane(s), c["Uin"], "the state after the stage dumps")
    s.advrk_step(0, P, c["method"], c["dt"])
    _same(_plane(s), c["new"], "new density, ghost frame included")


@pytest.mark.parametrize("k", range(NCASES))
def test_fused_step_equals_stage_by_stage(dev, golden, k):
    """pyrohip_advrk_step against RKIntegrator: pyrohip_state_lincomb for every stage start,
    ghost fill, pyrohip_advrk_rhs, the final pyrohip_state_lincomb -- bit for bit, ghost frame
    included"""
    c = _case(golden, k)
    P = _params(c)
    fused, start = _state(dev, c), _state(dev, c)
    fused.advrk_step(0, P, c["method"], c["dt"])
    rk = integration.RKIntegrator(0.0, c["dt"], method=c["method"])
    rk.set_start(start)
    assert rk.nstages() == c["ns"]
    for n in range(rk.nstages()):
        y = rk.get_stage_start(n)
        y.fill_bc(-1)
        y.advrk_rhs(0, P, rk.k, n)
        rk.store_increment(n)
    rk.compute_final_update()
    _same(_plane(fused), _plane(start), "fused step against the stage-by-stage path")
    _same(_plane(start), c["new"], "stage-by-stage path against the reference")


@pytest.mark.parametrize("k", range(NCASES))
def test_stages_contracted_build(dev, golden, k):
    c = _case(golden, k)
    s = _state(dev, c)
    s.advrk_step(0, _params(c, fast_math=1), c["method"], c["dt"])
    err = max_rel_err(_plane(s), c["new"])
    print(f"case {k}: contracted build, max_rel_err = {err:.3e} (reference's twin: {c['twin_dev']:.3e})")
    assert err <= 1e-12


@pytest.mark.parametrize("k", (1, 9))
@pytest.mark.parametrize("nsteps", (1, 2, 5))
def test_evolve_is_single_steps(dev, golden, k, nsteps):
    """pyrohip_advrk_evolve alternates between the state's plane and a work plane: odd and even
    step counts give, ghost frame included, what that many single steps give"""
    c = _case(golden, k)
    P = _params(c)
    dts = [c["dt"] * f for f in (1.0, 0.7, 0.9, 0.35, 0.8)][:nsteps]
    one, many = _state(dev, c), _state(dev, c)
    for dt in dts:
        one.advrk_step(0, P, c["method"], dt)
    many.advrk_evolve(0, P, c["method"], dts)
    _same(_plane(many), _plane(one), f"{nsteps} steps in one call")
    assert not np.array_equal(_plane(many), c["Uin"])


def test_work_area_survives_a_change_of_solver(dev):
    """A state's work area is one allocation that advection_rk (four planes), advection (one plane,
    exchanged with the state's own allocation where both have one plane) and every other solver
    use in turn.  The same four calls on ONE one-variable state and on a fresh state per call,
    uploaded with the previous result, give the same bits after every call, ghost frame included,
    in both builds: same kernels, same inputs.  8 x 8 is the smallest grid with room over the
    entry points' nx >= 4.  And a work area that another solver filled is no answer to "has the
    producer run": the compressible stage dump of a state on which only swe stepped is refused."""
    nx = ny = 8
    ng = 4
    dx = dy = 1.0 / nx
    x = (np.arange(nx + 2 * ng) - ng + 0.5) * dx
    X, Y = np.meshgrid(x, x, indexing="ij")
    a0 = 1.0 + 0.5 * np.sin(2 * np.pi * X) * np.cos(2 * np.pi * Y) + 0.25 * np.sin(4 * np.pi * (X + Y))
    dts = [0.4 * dx, 0.3 * dx]

    def fresh(a):
        s = device.DeviceState(dev, nx, ny, ng, [["periodic"] * 4])
        s.upload(np.ascontiguousarray(a[:, :, None]))
        return s

    for fast_math in (0, 1):
        P = _lib.AdvRkParams(dx, dy, 1.0, 1.0, 2, 2, fast_math)
        calls = (("advrk_evolve", lambda s: s.advrk_evolve(0, P, "RK4", dts)),
                 ("adv_step, fill folded in",
                  lambda s: s.adv_step(0, dx, dy, 1.0, 1.0, dts[0], 2, fill=True, fast_math=fast_math)),
                 ("advrk_evolve again", lambda s: s.advrk_evolve(0, P, "RK4", dts)),
                 ("adv_evolve", lambda s: s.adv_evolve(0, dx, dy, 1.0, 1.0, dts, 2, fast_math=fast_math)))
        one, prev = fresh(a0), a0
        for what, call in calls:
            call(one)
            each = fresh(prev)
            call(each)
            got, prev = _plane(one), _plane(each)
            assert not np.array_equal(prev[ng:-ng, ng:-ng], a0[ng:-ng, ng:-ng])
            _same(got, prev, f"fast_math {fast_math}, after {what}: one state against a fresh one per call")

    # refusals stay refusals
    h = np.zeros((nx + 2 * ng, ny + 2 * ng, 4))
    h[:, :, 0] = 1.0 + 0.1 * np.exp(-40.0 * ((X - 0.5) ** 2 + (Y - 0.5) ** 2))
    s = device.DeviceState(dev, nx, ny, ng, [["outflow"] * 4] * 4)
    s.upload(h)
    s.fill_bc()
    s.swe_step(dx, dy, 1.0, 2, "Roe", 0.1 * dx, kernel_set=0)     # (the staged set: it has work planes)
    s.swe_step(dx, dy, 1.0, 2, "Roe", 0.1 * dx)
    with pytest.raises(_lib.PyroHipError, match="no staged step has been run") as e:
        s.comp_stage("q")
    assert e.value.code == ERR_ARG


# ---- through the driver -----------------------------------------------------------------------

@pytest.fixture
def api(dev, tmp_path, monkeypatch):
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    return dev


def _pyro(scheme, nx, ny, nsteps, extra=None, problem="smooth", solver=None):
    from pyro2_amd.pyro_sim import Pyro
    p = solver or Pyro(SOLVER[scheme])
    over = {"gpu.fast_math": 0}
    if nx:
        over.update({"mesh.nx": nx, "mesh.ny": ny, "driver.max_steps": nsteps})
    over.update(extra or {})
    p.initialize_problem(problem, inputs_dict=over)
    return p


def _dens(p):
    return np.array(np.asarray(p.sim.cc_data.data)[:, :, 0])


@pytest.mark.parametrize("k", range(NCASES))
def test_timestep(api, golden, k):
    """method_compute_timestep: cfl / (max(|u|, SMALL) / dx + max(|v|, SMALL) / dy)"""
    c = _case(golden, k)
    sides = dict(zip(("mesh.xlboundary", "mesh.xrboundary", "mesh.ylboundary", "mesh.yrboundary"),
                     [b.replace("-even", "") for b in c["bc"]]))
    p = _pyro(c["scheme"], c["nx"], c["ny"], 1, dict(sides, **{"advection.u": c["u"], "advection.v": c["v"],
                                                              "driver.cfl": c["cfl"]}))
    g = p.sim.cc_data.grid
    assert (g.dx, g.dy) == (c["dx"], c["dy"])
    p.sim.method_compute_timestep()
    print("dt", p.sim.dt, c["dt"])
    assert p.sim.dt == c["dt"]


@pytest.mark.parametrize("path", ("batched", "single", "staged"))
@pytest.mark.parametrize("r", range(2))
@pytest.mark.parametrize("nsteps", (5, 20))
@pytest.mark.parametrize("scheme", (2, 4))
def test_short_runs(api, golden, scheme, r, nsteps, path):
    """5 and 20 steps of `smooth` through the driver (advection_fv4: preevolve included) by its
    batched path (evolve_many), by evolve() called singly, and by a subclass with a substep() of
    its own (stage by stage through RKIntegrator): time, step count and data equal the
    reference's"""
    from pyro2_amd.pyro_sim import Pyro
    g = golden("advrk_runs")
    nx, ny = GRIDS[r]
    solver = None
    if path == "staged":
        solver = Pyro(SOLVER[scheme])
        calls = []

        class Staged(solver.solver.Simulation):
            def substep(self, st, kstate, slot):
                calls.append(slot)
                super().substep(st, kstate, slot)
        solver.solver = type("solver", (), {"Simulation": Staged})
    p = _pyro(scheme, nx, ny, nsteps, solver=solver)
    assert p.sim.cc_data.names == ["density"]
    assert type(p.sim.cc_data).__name__ == ("FV2d" if scheme == 4 else "CellCenterData2d")
    if path == "batched":
        assert p.sim.can_evolve_many()
        p.run_sim()
    elif path == "single":
        while not p.sim.finished():
            p.single_step()
    else:
        assert not p.sim.can_evolve_many()
        p.run_sim()
        assert calls == [0, 1, 2, 3] * nsteps
    assert p.sim.n == nsteps and p.sim.cc_data.t == float(g[f"s{scheme}_r{r}_t{nsteps}"])
    ref = g[f"s{scheme}_r{r}_state{nsteps}"]
    # (the ghost frame: the fill at the start of the last step, as in the reference)
    _same(_dens(p), ref, f"{SOLVER[scheme]} {nx} x {ny}, {nsteps} steps, ghost frame included")


@pytest.mark.parametrize("batched", (True, False))
@pytest.mark.parametrize("scheme", (2, 4))
def test_particles(api, golden, scheme, batched):
    """tracer particles ride on the constant velocity: positions after 5 steps equal the
    reference's"""
    g = golden("advrk_runs")
    p = _pyro(scheme, 33, 36, 5, {"particles.do_particles": 1, "particles.n_particles": 25})
    if batched:
        assert p.sim.can_evolve_many()
        p.run_sim()
    else:
        while not p.sim.finished():
            p.single_step()
    _same(p.sim.particles.get_init_positions(), g[f"s{scheme}_part_init"], "initial positions")
    _same(p.sim.particles.get_positions(), g[f"s{scheme}_part_pos5"], "positions after 5 steps")
    I = (slice(4, -4), slice(4, -4))
    _same(_dens(p)[I], g[f"s{scheme}_part_state5"][I], "data")


@pytest.mark.parametrize("scheme", (2, 4))
def test_regression_smooth_0081(api, golden, scheme):
    """pyro/test.py's lines for these solvers: inputs.smooth to the end.  The bit-faithful build
    reproduces the reference's stored output file bit for bit; the contracted build stays within
    the reference's own sensitivity to 1e-15 noise on its initial data.
    The deviation of the contracted build is printed (-s); figures: DESIGN §12."""
    from pyro2_amd.util import h5pure
    p = _pyro(scheme, 0, 0, 0)
    p.run_sim()
    assert p.sim.n == 81
    with h5pure.File(os.path.join(GOLDEN, STORED[scheme])) as f:
        assert int(f.attrs["nsteps"]) == 81
        assert p.sim.cc_data.t == float(f.attrs["time"])
        stored = np.array(f["state"]["density"]["data"][:, :])
    _same(np.asarray(p.sim.cc_data.get_var("density").v()), stored, "density against the stored file")
    reg = golden("advrk_regress")
    pre = f"s{scheme}_"
    assert int(reg[pre + "n"]) == 81 and int(reg[pre + "twin_n"]) == 81
    assert np.array_equal(reg[pre + "density"], stored)      # the reference as it runs today
    q = _pyro(scheme, 0, 0, 0, {"gpu.fast_math": 1})
    q.run_sim()
    bar = max(10.0 * float(reg[pre + "twin_dev"]), 1e-12)
    err = max_rel_err(np.asarray(q.sim.cc_data.get_var("density").v()), stored)
    print(f"{SOLVER[scheme]}: contracted build after 81 steps: max_rel_err = {err:.3e}, twin_dev = "
          f"{float(reg[pre + 'twin_dev']):.3e}, bar = {bar:.3e}")
    assert q.sim.n == 81 and err <= bar


@pytest.mark.parametrize("scheme", (2, 4))
def test_output_file_and_restart(api, scheme, monkeypatch):
    """the file the driver writes has the stored file's groups, dataset names and attributes;
    io_pyro.read restores the Simulation class and the data class; a restarted run continues bit
    for bit and does not run preevolve again"""
    import importlib
    from pyro2_amd.pyro_sim import Pyro
    from pyro2_amd.util import h5pure, io_pyro
    Simulation = importlib.import_module("pyro2_amd." + SOLVER[scheme]).Simulation
    p = _pyro(scheme, 16, 19, 6, {"io.do_io": 1, "io.basename": "rk_", "io.n_out": 3, "io.dt_out": 1e33})
    p.run_sim()
    assert os.path.exists("rk_0003.h5") and os.path.exists("rk_0006.h5")
    with h5pure.File(os.path.join(GOLDEN, STORED[scheme])) as ref, h5pure.File("rk_0003.h5") as f:
        assert set(ref) <= set(f)
        assert list(f["state"]) == list(ref["state"]) == ["density"]
        for k in ("solver", "problem"):
            assert f.attrs[k] == ref.attrs[k] or f.attrs[k] == ref.attrs[k].decode()
        assert set(ref.attrs) <= set(f.attrs)
        assert int(f.attrs["nsteps"]) == 3
        assert set(ref["grid"].attrs) <= set(f["grid"].attrs)
        a, b = f["state"]["density"], ref["state"]["density"]
        assert list(a) == list(b) == ["data"]
        assert a["data"].shape == (16, 19) and a["data"].dtype == b["data"].dtype
        assert set(a.attrs) == set(b.attrs) == {"xlb", "xrb", "ylb", "yrb"}
        for k in a.attrs:
            assert a.attrs[k] == b.attrs[k]
    back = io_pyro.read("rk_0003.h5")
    assert type(back) is Simulation and back.n == 3
    assert type(back.cc_data).__name__ == ("FV2d" if scheme == 4 else "CellCenterData2d")
    # the stored file of the reference comes back the same way
    ref_back = io_pyro.read(os.path.join(GOLDEN, STORED[scheme]))
    assert type(ref_back) is Simulation and type(ref_back.cc_data) is type(back.cc_data)
    pre = []
    monkeypatch.setattr(Simulation, "preevolve", lambda self, _f=Simulation.preevolve: (pre.append(1), _f(self))[1])
    q = Pyro(SOLVER[scheme])
    q.restart_problem("rk_0003.h5", inputs_dict={"io.do_io": 0})
    assert q.sim.n == 3 and len(pre) == (0 if scheme == 4 else 1)
    assert np.array_equal(np.asarray(back.cc_data.get_var("density").v()),
                          np.asarray(q.sim.cc_data.get_var("density").v()))
    q.run_sim()
    assert q.sim.n == 6 and q.sim.cc_data.t == p.sim.cc_data.t
    I = (slice(4, -4), slice(4, -4))
    _same(_dens(q)[I], _dens(p)[I], "restarted run")


def test_refusals(api, golden, monkeypatch):
    """each of these fails with a message and without a launch"""
    c = _case(golden, 0)
    s = _state(api, c)
    before = _plane(s)
    lib = api._l

    def refused(call):
        with pytest.raises(_lib.PyroHipError) as e:
            call()
        assert e.value.code == ERR_ARG
        return str(e.value)

    dt, m = c["dt"], c["method"]
    assert "limiter" in refused(lambda: s.advrk_step(0, _params(c, limiter=10), m, dt))
    assert "limiter" in refused(lambda: s.advrk_evolve(0, _params(c, limiter=12), m, [dt, dt]))
    assert "limiter" in refused(lambda: s.advrk_step(0, _params(c, limiter=-1), m, dt))
    assert "scheme" in refused(lambda: s.advrk_step(0, _params(c, scheme=3), m, dt))
    assert "dx" in refused(lambda: s.advrk_step(0, _params(c, dx=0.0), m, dt))
    assert "index" in refused(lambda: s.advrk_step(1, _params(c), m, dt))
    with pytest.raises(ValueError, match="temporal method"):
        s.advrk_step(0, _params(c), "RK3", dt)
    rc = lib.pyrohip_advrk_step(s.h, 0, _params(c), 7, dt)
    assert rc == ERR_ARG and b"temporal method" in lib.pyrohip_last_error()
    assert lib.pyrohip_advrk_step(s.h, 0, None, 3, dt) == ERR_ARG
    assert lib.pyrohip_advrk_step(None, 0, _params(c), 3, dt) == ERR_ARG
    assert lib.pyrohip_advrk_evolve(s.h, 0, _params(c), 3, None, 2) == ERR_ARG
    k = _state(api, c)
    assert "slot" in refused(lambda: s.advrk_rhs(0, _params(c), k, 1))
    assert "of their own" in refused(lambda: s.advrk_rhs(0, _params(c), s, 0))
    # a limiter >= 10 is a setting of the fourth-order scheme like any other non-zero one
    s4 = _state(api, c)
    s4.advrk_step(0, _params(c, scheme=4, limiter=10), m, dt)
    assert np.array_equal(_plane(s), before)
    for ng in (3, 5):
        t = _state(api, dict(c, nx=8, ny=8), ng=ng)
        assert "ng = 4" in refused(lambda: t.advrk_step(0, _params(c), m, dt))
        assert "ng = 4" in refused(lambda: t.advrk_rhs(0, _params(c), t, 0))
    for side, kind in ((0, "reflect-odd"), (1, "reflect-odd"), (2, "reflect-odd"), (3, "reflect-odd"),
                       (3, "moving_lid")):
        bc = list(c["bc"])
        bc[side] = kind
        t = _state(api, dict(c, nx=8, ny=8), bc=bc, ng=4)
        assert "boundaries only" in refused(lambda: t.advrk_step(0, _params(c), m, dt))

    # through the driver
    def start(scheme, extra):
        _pyro(scheme, 16, 16, 1, extra)

    with pytest.raises((SystemExit, ValueError)):
        start(2, {"advection.limiter": 10})
    with pytest.raises((SystemExit, ValueError)):
        start(2, {"advection.temporal_method": "RK3"})
    with pytest.raises((SystemExit, ValueError)):
        start(4, {"advection.temporal_method": "euler"})
    from pyro2_amd import decomp
    for scheme in (2, 4):
        with pytest.raises(RuntimeError, match="one process only"):
            start(scheme, {"gpu.decompose": 1})
    # an active decomposition (two ranks, no transport: nothing may be sent)
    monkeypatch.setattr(decomp, "_current", decomp.Decomposition(lambda ctx: None, 0, 2))
    for scheme in (2, 4):
        with pytest.raises((SystemExit, ValueError)):
            start(scheme, {})


@pytest.mark.parametrize("scheme", (2, 4))
def test_no_field_traffic_in_a_batched_run(api, scheme, monkeypatch):
    """once the data are on the device, a batched run moves no field between host and device:
    neither the DeviceState transfer methods nor their C functions are called"""
    p = _pyro(scheme, 16, 19, 12)
    assert p.sim.can_evolve_many() and len(p.sim.evolve_many(2)) == 2
    calls = []
    for n in ("upload", "download", "upload_rows", "download_rows", "upload_var", "download_var",
              "advrk_stages"):
        def spy(self, *a, _n=f"DeviceState.{n}", _f=getattr(device.DeviceState, n), **kw):
            calls.append(_n)
            return _f(self, *a, **kw)
        monkeypatch.setattr(device.DeviceState, n, spy)
    lib = api._l
    for n in ("pyrohip_state_upload", "pyrohip_state_download", "pyrohip_state_upload_rows",
              "pyrohip_state_download_rows", "pyrohip_state_upload_var", "pyrohip_state_download_var",
              "pyrohip_advrk_stage_dump"):
        def cspy(*a, _n=n, _f=getattr(lib, n)):
            calls.append(_n)
            return _f(*a)
        monkeypatch.setattr(lib, n, cspy, raising=False)
    p.run_sim()
    assert p.sim.n == 12 and not calls, calls
    # positive control: the spies do see a transfer
    p.sim.cc_data.device_state().download()
    assert calls == ["DeviceState.download", "pyrohip_state_download"], calls


def test_solvers_are_registered():
    import pyro
    from pyro2_amd import pyro_sim
    assert {"advection_rk", "advection_fv4"} <= set(pyro_sim.valid_solvers)
    import pyro.advection_fv4.simulation as fv4
    import pyro.advection_rk.simulation as rk
    from pyro.advection_fv4.problems import smooth
    from pyro.advection_rk.problems import tophat
    import pyro2_amd.advection.problems.smooth as real_smooth
    import pyro2_amd.advection_rk.simulation as real
    assert rk is real and issubclass(fv4.Simulation, rk.Simulation) and pyro.__name__ == "pyro"
    assert smooth is real_smooth and callable(tophat.init_data)
