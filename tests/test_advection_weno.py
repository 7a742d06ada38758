"""advection_weno (method-of-lines advection of a scalar with a constant velocity, WENO
reconstructions of order 2 or 3 of Lax-Friedrichs split fluxes) on the device against runs of the
reference (tools/gen_advweno_golden.py): the WENO flux of the stage kernel of
csrc/advection_rk.hip (pyrohip_advrk_params.scheme = 5) stage by stage, the fused Runge-Kutta step
against the stage-by-stage path, the several-steps call, short runs through the driver, the run of
`smooth` to t = 1, the output files this package writes, tracer particles and the refusals.

Tolerances.  The bit-faithful build (gpu.fast_math = 0: no FMA contraction but the one chain of
fused multiply-adds that np.dot is in the reference, the reference's operation order, true
divisions) is held to equality, ghost frame included.  The contracted build is held to the
project's advection tolerance, 1e-12 by conftest.max_rel_err, for one step (the reference's own
step moves by less than 1e-14 under 1e-15 relative noise on its input in every recorded case but
those with structure of 1e-4 on a constant, where beta^2 is of the size of the 1e-16 beside it:
`twin_dev` of advweno_stages.npz, asserted <= 1e-12 by the generator for every other case; a
small-structure case whose twin_dev is above 1e-12 is held to 10 x its twin_dev); for the 81
steps of the runs to t = 1 to max(10 x twin_dev, 1e-12), twin_dev being what a run of the
reference with 1e-15 relative noise on its initial data differs by from the clean one
(advweno_regress.npz; measured figures: DESIGN §13)."""
import os

import numpy as np
import pytest

from conftest import max_rel_err
from pyro2_amd import _lib, device
from pyro2_amd.mesh import integration

NCASES = 14
ERR_ARG = 10001
RUNS = ((0, (33, 36), 5), (1, (16, 19), 5), (1, (16, 19), 20))
PLANES = ("start", "fpr_x", "fpr_y", "F_x", "F_y", "k")


def _case(golden, k):
    g = golden("advweno_stages")
    assert int(g["ncases"]) == NCASES
    pre = f"c{k}_"
    m = g[pre + "meta"]
    c = {"nx": int(m[0]), "ny": int(m[1]), "ng": int(m[2]), "order": int(m[3]), "scheme": int(m[4]),
         "dx": float(m[5]), "dy": float(m[6]), "u": float(m[7]), "v": float(m[8]), "cfl": float(m[9]),
         "ns": int(m[10]), "alpha": float(m[11]), "amp": float(m[12]), "method": str(g[pre + "method"]),
         "data": str(g[pre + "data"]), "bc": [str(b) for b in g[pre + "bc"]],
         "Uin": g[pre + "Uin"], "new": g[pre + "new"], "dt": float(g[pre + "dt"]),
         "dt_method": float(g[pre + "dt_method"]), "twin_dev": float(g[pre + "twin_dev"])}
    c["stages"] = [{key: g[f"{pre}s{s}_{key}"] for key in PLANES} for s in range(c["ns"])]
    return c


def _state(dev, c):
    s = device.DeviceState(dev, c["nx"], c["ny"], c["ng"], [c["bc"]])
    s.upload(np.ascontiguousarray(c["Uin"][:, :, None]))
    return s


def _plane(s):
    return np.ascontiguousarray(s.download()[:, :, 0])


def _params(c, fast_math=0, **over):
    kw = dict(dx=c["dx"], dy=c["dy"], u=c["u"], v=c["v"], scheme=5, weno_order=c["order"], alpha=c["alpha"])
    kw.update(over)
    P = _lib.AdvRkParams(kw["dx"], kw["dy"], kw["u"], kw["v"], 0, kw["scheme"], fast_math)
    P.weno_order, P.alpha = kw["weno_order"], kw["alpha"]
    return P


def _same(got, ref, what):
    d = np.abs(np.asarray(got) - np.asarray(ref)).max()
    print(f"{what}: max |diff| = {d:.3e}, max |ref| = {np.abs(ref).max():.3e}")
    assert np.array_equal(got, ref), (what, d)


def _moves(c):
    """does the step change the interior?  Not at zero velocity, not on an exactly constant field"""
    return (c["u"], c["v"]) != (0.0, 0.0) and not (c["data"] == "constant" and c["amp"] == 0.0)


def test_cases_cover_the_issue(golden):
    """the recorded cases: both orders, every method, the three boundary kinds, the velocities
    (zero and negative components, zero altogether), the grids from several ragged tiles down to
    4 x 5, where the stencil of order 3 wraps the periodic grid, dx != dy, and the kinds of data"""
    cs = [_case(golden, k) for k in range(NCASES)]
    assert all(c["scheme"] == 5 and c["ng"] == 4 for c in cs)
    assert {c["order"] for c in cs} == {2, 3}
    assert {(c["order"], c["method"]) for c in cs} >= {(o, m) for o in (2, 3) for m in ("RK2", "TVD2", "RK4")}
    assert {c["method"] for c in cs} == {"RK2", "TVD2", "TVD3", "RK4"}
    assert {b for c in cs for b in c["bc"]} == {"periodic", "outflow", "reflect-even"}
    assert any(c["bc"][:2] == ["reflect-even"] * 2 for c in cs) and any(c["bc"][2:] == ["reflect-even"] * 2 for c in cs)
    assert {(c["nx"], c["ny"]) for c in cs} >= {(33, 36), (16, 19), (19, 16), (8, 8), (4, 5)}
    assert any((c["nx"], c["ny"], c["order"]) == (4, 5, 3) and c["bc"] == ["periodic"] * 4 for c in cs)
    assert {(c["u"], c["v"]) for c in cs} >= {(1.0, 1.0), (-1.0, 0.5), (0.7, -1.0), (0.0, 1.0), (-1.0, 0.0),
                                             (0.0, 0.0)}
    assert any(c["dx"] != c["dy"] for c in cs)
    assert {(c["data"], c["amp"]) for c in cs} >= {("smooth", 1.0), ("tophat", 0.0), ("constant", 0.0),
                                                  ("constant", 1e-4)}
    for c in cs:
        assert c["alpha"] == np.sqrt(c["u"]**2 + c["v"]**2)
        ng = c["ng"]
        inner = (slice(ng, -ng), slice(ng, -ng))
        # junk in the ghost cells of the input: the step has to apply the boundary rules itself
        assert not np.array_equal(c["Uin"], c["stages"][0]["start"])
        assert np.array_equal(c["Uin"][inner], c["stages"][0]["start"][inner])
        if (c["u"], c["v"]) == (0.0, 0.0):
            assert c["alpha"] == 0.0 and np.array_equal(c["new"][inner], c["Uin"][inner])
    assert all(c["twin_dev"] <= 1e-12 or (c["data"] == "constant" and 0.0 < c["amp"] <= 1e-4 and
                                           c["twin_dev"] <= 1e-10) for c in cs)
    assert [f[0] for f in _lib.AdvRkParams._fields_][-2:] == ["weno_order", "alpha"]


@pytest.mark.parametrize("k", range(NCASES))
def test_stages_bit_for_bit(dev, golden, k):
    """one evolve() of the reference per case, from a plane whose ghost cells hold junk.  Per
    stage the stage start with its ghost cells, the reconstructed positive part of the split flux
    and the fluxes on the faces the update reads and k_s, then the new density with its ghost
    frame: equal to the reference's, bit for bit."""
    c = _case(golden, k)
    ng, nx, ny = c["ng"], c["nx"], c["ny"]
    s = _state(dev, c)
    P = _params(c)
    fx = (slice(ng, ng + nx + 1), slice(ng, ng + ny))
    fy = (slice(ng, ng + nx), slice(ng, ng + ny + 1))
    inner = (slice(ng, ng + nx), slice(ng, ng + ny))
    for n, ref in enumerate(c["stages"]):
        st = s.advrk_stages(0, P, c["method"], c["dt"], n)
        _same(st[5], ref["start"], f"stage {n}: stage start, ghost cells included")
        _same(st[0][fx], ref["fpr_x"][fx], f"stage {n}: flux_p_r, x")
        _same(st[1][fy], ref["fpr_y"][fy], f"stage {n}: flux_p_r, y")
        _same(st[2][fx], ref["F_x"][fx], f"stage {n}: F_x")
        _same(st[3][fy], ref["F_y"][fy], f"stage {n}: F_y")
        _same(st[4][inner], ref["k"][inner], f"stage {n}: k")
        assert (np.abs(ref["k"][inner]).max() > 0.0) == _moves(c)
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
    """the contracted build (FMA contraction, one reciprocal of sum(alpha), reciprocals of dx and
    dy): one step within 1e-12 of the reference's -- within 10 x twin_dev in a case of small
    structure on a constant whose twin_dev is itself above 1e-12 (no other case may be)"""
    c = _case(golden, k)
    s = _state(dev, c)
    s.advrk_step(0, _params(c, fast_math=1), c["method"], c["dt"])
    err = max_rel_err(_plane(s), c["new"])
    bar = 1e-12 if c["twin_dev"] <= 1e-12 else 10.0 * c["twin_dev"]
    print(f"case {k}: contracted build, max_rel_err = {err:.3e} (reference's twin: {c['twin_dev']:.3e}, "
          f"bar {bar:.1e})")
    assert err <= bar


@pytest.mark.parametrize("k", (1, 2))
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


def test_other_schemes_ignore_the_new_fields(dev, golden):
    """schemes 2 and 4 do not read weno_order and alpha: junk there changes nothing"""
    c = _case(golden, 1)
    for scheme in (2, 4):
        a, b = _state(dev, c), _state(dev, c)
        P = _lib.AdvRkParams(c["dx"], c["dy"], c["u"], c["v"], 1, scheme, 0)
        assert (P.weno_order, P.alpha) == (0, 0.0)
        a.advrk_step(0, P, "RK4", c["dt"])
        P.weno_order, P.alpha = 7, float("nan")
        b.advrk_step(0, P, "RK4", c["dt"])
        _same(_plane(b), _plane(a), f"scheme {scheme}")


# ---- through the driver -----------------------------------------------------------------------

@pytest.fixture
def api(dev, tmp_path, monkeypatch):
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    return dev


def _pyro(order, nx, ny, nsteps, extra=None, problem="smooth", solver=None):
    from pyro2_amd.pyro_sim import Pyro
    p = solver or Pyro("advection_weno")
    over = {"gpu.fast_math": 0, "advection.weno_order": order}
    if nx:
        over.update({"mesh.nx": nx, "mesh.ny": ny, "driver.max_steps": nsteps})
    over.update(extra or {})
    p.initialize_problem(problem, inputs_dict=over)
    return p


def _dens(p):
    return np.array(np.asarray(p.sim.cc_data.data)[:, :, 0])


def test_defaults(api):
    """the reference's parameter names and default values"""
    from pyro2_amd.pyro_sim import Pyro
    rp = Pyro("advection_weno").rp
    assert [rp.get_param("advection." + k) for k in ("u", "v", "limiter", "weno_order", "temporal_method")] == \
        [1.0, 1.0, 0, 3, "RK4"]
    assert rp.get_param("driver.cfl") == 0.5


@pytest.mark.parametrize("k", range(NCASES))
def test_timestep_and_params(api, golden, k):
    """method_compute_timestep: cfl / (max(|u|, SMALL) / dx + max(|v|, SMALL) / dy); the
    parameters handed to the device: scheme 5, the order, alpha as the reference forms it"""
    c = _case(golden, k)
    sides = dict(zip(("mesh.xlboundary", "mesh.xrboundary", "mesh.ylboundary", "mesh.yrboundary"),
                     [b.replace("-even", "") for b in c["bc"]]))
    p = _pyro(c["order"], c["nx"], c["ny"], 1, dict(sides, **{"advection.u": c["u"], "advection.v": c["v"],
                                                             "driver.cfl": c["cfl"]}))
    g = p.sim.cc_data.grid
    assert (g.dx, g.dy, g.ng) == (c["dx"], c["dy"], 4)
    p.sim.method_compute_timestep()
    print("dt", p.sim.dt, c["dt_method"])
    assert p.sim.dt == c["dt_method"]
    P = p.sim._params()
    assert (P.scheme, P.weno_order, P.alpha, P.fast_math) == (5, c["order"], c["alpha"], 0)


@pytest.mark.parametrize("path", ("batched", "single", "staged"))
@pytest.mark.parametrize("run", range(len(RUNS)))
@pytest.mark.parametrize("order", (2, 3))
def test_short_runs(api, golden, order, run, path):
    """5 and 20 steps of `smooth` through the driver by its batched path (evolve_many), by
    evolve() called singly, and by a subclass with a substep() of its own (stage by stage through
    RKIntegrator): time, step count and data equal the reference's"""
    from pyro2_amd.pyro_sim import Pyro
    g = golden("advweno_runs")
    r, (nx, ny), nsteps = RUNS[run]
    solver = None
    if path == "staged":
        solver = Pyro("advection_weno")
        calls = []

        class Staged(solver.solver.Simulation):
            def substep(self, st, kstate, slot):
                calls.append(slot)
                super().substep(st, kstate, slot)
        solver.solver = type("solver", (), {"Simulation": Staged})
    p = _pyro(order, nx, ny, nsteps, solver=solver)
    assert p.sim.cc_data.names == ["density"] and type(p.sim.cc_data).__name__ == "CellCenterData2d"
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
    assert p.sim.n == nsteps and p.sim.cc_data.t == float(g[f"o{order}_r{r}_t{nsteps}"])
    _same(_dens(p), g[f"o{order}_r{r}_state{nsteps}"], f"order {order}, {nx} x {ny}, {nsteps} steps, ghost frame included")


@pytest.mark.parametrize("batched", (True, False))
@pytest.mark.parametrize("order", (2, 3))
def test_particles(api, golden, order, batched):
    """tracer particles ride on the constant velocity: positions after 5 steps equal the
    reference's"""
    g = golden("advweno_runs")
    p = _pyro(order, 33, 36, 5, {"particles.do_particles": 1, "particles.n_particles": 25})
    if batched:
        assert p.sim.can_evolve_many()
        p.run_sim()
    else:
        while not p.sim.finished():
            p.single_step()
    _same(p.sim.particles.get_init_positions(), g[f"o{order}_part_init"], "initial positions")
    _same(p.sim.particles.get_positions(), g[f"o{order}_part_pos5"], "positions after 5 steps")
    I = (slice(4, -4), slice(4, -4))
    _same(_dens(p)[I], g[f"o{order}_r0_state5"][I], "data")


@pytest.mark.parametrize("order", (2, 3))
def test_regression_smooth(api, golden, order):
    """`smooth` with inputs.smooth to t = 1 (32 x 32, 81 steps).  The bit-faithful build
    reproduces the reference's run bit for bit, time and step count included; the contracted
    build stays within max(10 x twin_dev, 1e-12), twin_dev being the reference's own sensitivity
    to 1e-15 noise on its initial data.  The deviation of the contracted build is printed (-s);
    figures: DESIGN §13."""
    reg = golden("advweno_regress")
    pre = f"o{order}_"
    n, t, twin_n, twin_dev = reg[pre + "meta"]
    assert n == 81 and twin_n == 81
    p = _pyro(order, 0, 0, 0)
    p.run_sim()
    assert p.sim.n == 81 and p.sim.cc_data.t == t
    _same(np.asarray(p.sim.cc_data.get_var("density").v()), reg[pre + "density"], "density after 81 steps")
    q = _pyro(order, 0, 0, 0, {"gpu.fast_math": 1})
    q.run_sim()
    bar = max(10.0 * float(twin_dev), 1e-12)
    err = max_rel_err(np.asarray(q.sim.cc_data.get_var("density").v()), reg[pre + "density"])
    print(f"advection_weno order {order}: contracted build after 81 steps: max_rel_err = {err:.3e}, twin_dev = "
          f"{float(twin_dev):.3e}, bar = {bar:.3e}")
    assert q.sim.n == 81 and err <= bar


def test_output_file_and_restart(api):
    """the file the driver writes names the solver and holds the one variable; io_pyro.read
    restores the Simulation class; a restarted run continues bit for bit"""
    from pyro2_amd.advection_weno import Simulation
    from pyro2_amd.pyro_sim import Pyro
    from pyro2_amd.util import h5pure, io_pyro
    p = _pyro(3, 16, 19, 6, {"io.do_io": 1, "io.basename": "weno_", "io.n_out": 3, "io.dt_out": 1e33})
    p.run_sim()
    assert os.path.exists("weno_0003.h5") and os.path.exists("weno_0006.h5")
    with h5pure.File("weno_0003.h5") as f:
        solver = f.attrs["solver"]
        assert (solver.decode() if isinstance(solver, bytes) else solver) == "advection_weno"
        assert int(f.attrs["nsteps"]) == 3 and list(f["state"]) == ["density"]
        assert f["state"]["density"]["data"].shape == (16, 19)
    back = io_pyro.read("weno_0003.h5")
    assert type(back) is Simulation and back.n == 3 and type(back.cc_data).__name__ == "CellCenterData2d"
    q = Pyro("advection_weno")
    q.restart_problem("weno_0003.h5", inputs_dict={"io.do_io": 0})
    assert q.sim.n == 3 and q.sim.rp.get_param("advection.weno_order") == 3
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

    def refused(call):
        with pytest.raises(_lib.PyroHipError) as e:
            call()
        assert e.value.code == ERR_ARG
        return str(e.value)

    dt, m = c["dt"], c["method"]
    k = _state(api, c)
    for order in (1, 4, 0, -3):
        assert "weno_order" in refused(lambda: s.advrk_step(0, _params(c, weno_order=order), m, dt))
        assert "weno_order" in refused(lambda: s.advrk_evolve(0, _params(c, weno_order=order), m, [dt, dt]))
        assert "weno_order" in refused(lambda: s.advrk_rhs(0, _params(c, weno_order=order), k, 0))
        assert "weno_order" in refused(lambda: s.advrk_stages(0, _params(c, weno_order=order), m, dt, 0))
    for alpha in (-1.0, float("nan"), float("inf")):
        assert "alpha" in refused(lambda: s.advrk_step(0, _params(c, alpha=alpha), m, dt))
    assert "scheme" in refused(lambda: s.advrk_step(0, _params(c, scheme=3), m, dt))
    assert "scheme" in refused(lambda: s.advrk_step(0, _params(c, scheme=6), m, dt))
    assert "dx" in refused(lambda: s.advrk_step(0, _params(c, dx=0.0), m, dt))
    with pytest.raises(ValueError, match="temporal method"):
        s.advrk_step(0, _params(c), "RK3", dt)
    assert np.array_equal(_plane(s), before)
    bc = list(c["bc"])
    bc[2] = "reflect-odd"
    t = _state(api, dict(c, bc=bc))
    assert "boundaries only" in refused(lambda: t.advrk_step(0, _params(c), m, dt))

    # through the driver
    def start(extra):
        _pyro(3, 16, 16, 1, extra)

    for order in (1, 4):
        with pytest.raises((SystemExit, ValueError)):
            start({"advection.weno_order": order})
    with pytest.raises((SystemExit, ValueError)):
        start({"advection.temporal_method": "RK3"})
    from pyro2_amd import decomp
    with pytest.raises(RuntimeError, match="one process only"):
        start({"gpu.decompose": 1})
    # an active decomposition (two ranks, no transport: nothing may be sent)
    monkeypatch.setattr(decomp, "_current", decomp.Decomposition(lambda ctx: None, 0, 2))
    with pytest.raises((SystemExit, ValueError)):
        start({})


def test_no_field_traffic_in_a_batched_run(api, monkeypatch):
    """once the data are on the device, a batched run moves no field between host and device"""
    p = _pyro(3, 16, 19, 12)
    assert p.sim.can_evolve_many() and len(p.sim.evolve_many(2)) == 2
    calls = []
    for n in ("upload", "download", "upload_rows", "download_rows", "upload_var", "download_var", "advrk_stages"):
        def spy(self, *a, _n=f"DeviceState.{n}", _f=getattr(device.DeviceState, n), **kw):
            calls.append(_n)
            return _f(self, *a, **kw)
        monkeypatch.setattr(device.DeviceState, n, spy)
    p.run_sim()
    assert p.sim.n == 12 and not calls, calls
    p.sim.cc_data.device_state().download()
    assert calls == ["DeviceState.download"], calls


def test_solver_is_registered():
    import pyro
    from pyro2_amd import pyro_sim
    assert "advection_weno" in pyro_sim.valid_solvers
    import pyro.advection_rk.simulation as rk
    import pyro.advection_weno.simulation as weno
    from pyro.advection_weno.problems import smooth, tophat
    import pyro2_amd.advection.problems.smooth as real_smooth
    import pyro2_amd.advection_weno.simulation as real
    assert weno is real and issubclass(weno.Simulation, rk.Simulation) and pyro.__name__ == "pyro"
    assert weno.Simulation.scheme == 5
    assert smooth is real_smooth and callable(tophat.init_data)
