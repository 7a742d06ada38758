"""compressible_fv4 / compressible_sdc: the 4th-order right-hand side (pyrohip_comp_fv4_rhs),
cell averages <-> centres, the SDC node update and the two solvers through Pyro, against
fixtures of the reference (tools/gen_fv4_golden.py).  The `dev` tests run on the emulated
build here and on the MI355X under -m gpu."""
import numpy as np
import pytest

NAMES = ("density", "energy", "x-momentum", "y-momentum")


@pytest.fixture
def api(dev, tmp_path, monkeypatch):
    from pyro2_amd import device
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    return dev


def _rel(a, b):
    """per variable max |a - b| / max |b|"""
    return [float(np.abs(a[..., n] - b[..., n]).max() / max(np.abs(b[..., n]).max(), 1e-300))
            for n in range(a.shape[-1])]


def _rhs(ctx, U, bcs, meta, fast, slot=0, small_dens=-1.e200, heat=None, state=False):
    """k of U into slot `slot` of a k state pre-filled with 7.0; heat = (rate, profile);
    state=True also returns the stage state after the call"""
    from pyro2_amd import device
    qx, qy = U.shape[:2]
    nx, ny = qx - 8, qy - 8
    dx, dy, gamma, grav, flat, sponge, rb, rf, tau = meta
    P = device.make_comp_params(dx, dy, gamma=gamma, grav=grav, use_flattening=int(flat),
                                fast_math=fast, riemann="CGF", small_dens=small_dens,
                                sponge=(rb, rf, tau) if sponge else None,
                                heat_rate=heat[0] if heat is not None else 0.0)
    s = device.DeviceState(ctx, nx, ny, 4, [[str(b) for b in r] for r in bcs])
    s.upload(np.ascontiguousarray(U))
    if heat is not None:
        s.set_heating(heat[1])
    k = device.DeviceState(ctx, nx, ny, 4, [["outflow"] * 4] * (4 * (slot + 1)))
    k.upload(np.full((qx, qy, 4 * (slot + 1)), 7.0))
    s.comp_fv4_rhs(P, k, slot)
    got = k.download()[..., 4 * slot:4 * slot + 4]
    return (got, s.download()) if state else got


def _rhs_cases(golden):
    """(file, case) of every reference right-hand side: the three of comp_fv4_rhs and the
    ragged / sub-tile / dx != dy / heating / quad / density-floor cases of comp_fv4_edges"""
    return [(name, str(c)) for name in ("comp_fv4_rhs", "comp_fv4_edges") for c in golden(name)["cases"]]


def _case_args(g, case):
    """small_dens and (heat_rate, profile) of a fixture case (defaults where absent)"""
    sd = float(g[f"{case}_small_dens"]) if f"{case}_small_dens" in g else -1.e200
    heat = (float(g[f"{case}_heat_rate"]), g[f"{case}_heat"]) if f"{case}_heat" in g else None
    return sd, heat


# Variables whose k is zero analytically in a case: sod.x is uniform in y with reflecting y
# walls, so k of the y-momentum is round-off (max |k| 1.6e-10 against 11.4 for the x-momentum).
# Its error is measured against the momentum's scale, max |k| of both components.
ZERO_K = {("comp_fv4_edges", "sodx"): 3}


@pytest.mark.parametrize("fast,tol", [(0, 1e-14), (1, 1e-10)])
def test_fv4_rhs_vs_reference(dev, golden, fast, tol):
    """Simulation.substep of the reference: the acoustic pulse (32^2), a shocked sod state
    (32 x 48), rt with gravity and the sponge (24 x 40), and comp_fv4_edges: sod.x 21 x 13
    with a density floor above the outflow ghosts' density, rt 13 x 70 (hse), heating 18^2
    (a strong source), quad 20^2 and the pulse with dy = 1.5 dx.  Where the fixture holds the state after the
    call, the stage state must match it bit for bit (clean_state floors the interior only)."""
    for name, case in _rhs_cases(golden):
        g = golden(name)
        U, k, bcs, meta = g[f"{case}_U"], g[f"{case}_k"], g[f"{case}_bcs"], g[f"{case}_meta"]
        sd, heat = _case_args(g, case)
        got, Uout = _rhs(dev, U, bcs, meta, fast, slot=1, small_dens=sd, heat=heat, state=True)
        err = _rel(got[4:-4, 4:-4], k[4:-4, 4:-4])
        if (name, case) in ZERO_K:
            n, K = ZERO_K[(name, case)], k[4:-4, 4:-4]
            err[n] = float(np.abs(got[4:-4, 4:-4, n] - K[..., n]).max() / np.abs(K[..., 2:4]).max())
        print(name, case, "fast" if fast else "exact", err)
        assert max(err) <= tol, (case, err)
        if f"{case}_Uout" in g:
            assert np.array_equal(Uout, g[f"{case}_Uout"]), case


def test_fv4_from_to_centers(api):
    """FV2d.from_centers (device) and to_centers (host) against the formulas of mesh/fv.py,
    periodic and outflow boundaries"""
    from pyro2_amd.mesh import boundary as bnd
    from pyro2_amd.mesh import fv, patch
    rng = np.random.default_rng(3)
    for kind in ("periodic", "outflow"):
        g = patch.Grid2d(24, 40, ng=4, xmax=0.6, ymax=1.0)
        d = fv.FV2d(g)
        d.register_var("a", bnd.BC(xlb=kind, xrb=kind, ylb=kind, yrb=kind))
        d.create()
        a0 = 1.0 + rng.random((g.qx, g.qy))
        d.get_var("a")[:, :] = a0
        d.from_centers("a")
        got = np.array(d.get_var("a"))
        # numpy: ghost fill, then a + dx^2 lap / 24 on the interior
        ref = patch.CellCenterData2d(g)
        ref.register_var("a", bnd.BC(xlb=kind, xrb=kind, ylb=kind, yrb=kind))
        ref.create()
        ref.get_var("a")[:, :] = a0
        ref.fill_BC("a")
        b = np.array(ref.get_var("a"))
        lap = (b[:-2, 1:-1] - 2 * b[1:-1, 1:-1] + b[2:, 1:-1]) / g.dx**2 + \
              (b[1:-1, :-2] - 2 * b[1:-1, 1:-1] + b[1:-1, 2:]) / g.dy**2
        want = b.copy()
        want[1:-1, 1:-1] = b[1:-1, 1:-1] + g.dx**2 * lap / 24.0
        assert np.array_equal(got[4:-4, 4:-4], want[4:-4, 4:-4]), kind
        c = np.array(d.to_centers("a"))
        a = got
        lap = (a[:-2, 1:-1] - 2 * a[1:-1, 1:-1] + a[2:, 1:-1]) / g.dx**2 + \
              (a[1:-1, :-2] - 2 * a[1:-1, 1:-1] + a[1:-1, 2:]) / g.dy**2
        wc = a.copy()
        wc[1:-1, 1:-1] = a[1:-1, 1:-1] - g.dx**2 * lap / 24.0
        assert np.array_equal(c, wc), kind


@pytest.mark.parametrize("fast,tol", [(0, 1e-12), (1, 1e-10)])
@pytest.mark.parametrize("solver,steps", [("compressible_fv4", 4), ("compressible_sdc", 3)])
def test_fv4_sdc_runs_vs_reference(api, golden, solver, steps, fast, tol):
    """a few steps of each solver through Pyro (CFL steps of the driver) on the 32^2 pulse"""
    from pyro2_amd.pyro_sim import Pyro
    g = golden("comp_fv4_runs")
    p = Pyro(solver)
    p.initialize_problem("acoustic_pulse", inputs_file="inputs.acoustic_pulse",
                         inputs_dict={"mesh.nx": 32, "mesh.ny": 32, "driver.fix_dt": -1.0,
                                      "driver.max_steps": steps, "gpu.fast_math": fast})
    dts = []
    for _ in range(steps):
        p.single_step()
        dts.append(p.sim.dt)
    assert np.abs(np.array(dts) - g[solver + "_dts"]).max() <= 1e-12 * g[solver + "_dts"].max()
    U = np.array(p.sim.cc_data.data)
    err = _rel(U[4:-4, 4:-4], g[solver + "_U"][4:-4, 4:-4])
    print(solver, fast, err)
    assert max(err) <= tol


@pytest.mark.parametrize("fast,tol", [(0, 1e-12), (1, 1e-10)])
@pytest.mark.parametrize("solver,steps", [("compressible_fv4", 4), ("compressible_sdc", 3)])
@pytest.mark.parametrize("grid", ["sodx", "rt"])
def test_fv4_sdc_edge_runs_vs_reference(api, golden, grid, solver, steps, fast, tol):
    """the same on ragged, non-periodic grids: sod.x at 44 x 12 (outflow x, reflect y) and rt at
    12 x 36 (periodic x, hse y, gravity) -- boundary fill, stages and SDC node updates"""
    from pyro2_amd.pyro_sim import Pyro
    g = golden("comp_fv4_edge_runs")
    prob, inputs, extra = {
        "sodx": ("sod", "inputs.sod.x", {"mesh.nx": 44, "mesh.ny": 12, "mesh.xmax": 1.0, "mesh.ymax": 12 / 44}),
        "rt": ("rt", "inputs.rt", {"mesh.nx": 12, "mesh.ny": 36, "mesh.xmax": 0.5, "mesh.ymax": 1.5})}[grid]
    p = Pyro(solver)
    p.initialize_problem(prob, inputs_file=inputs,
                         inputs_dict=dict(extra, **{"driver.fix_dt": -1.0, "driver.max_steps": steps,
                                                    "gpu.fast_math": fast}))
    dts = []
    for _ in range(steps):
        p.single_step()
        dts.append(p.sim.dt)
    pre = f"{grid}_{solver}"
    assert np.abs(np.array(dts) - g[pre + "_dts"]).max() <= 1e-12 * g[pre + "_dts"].max()
    U = np.array(p.sim.cc_data.data)
    err = _rel(U[4:-4, 4:-4], g[pre + "_U"][4:-4, 4:-4])
    print(grid, solver, fast, err)
    assert max(err) <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("solver", ["compressible_fv4", "compressible_sdc"])
def test_fv4_sdc_reference_regression(hip, golden, tmp_path, monkeypatch, solver, fast):
    """pyro/test.py:104-107 -- acoustic_pulse inputs.acoustic_pulse (128^2, 160 steps to t = 0.24)
    against the stored acoustic_pulse_0160.h5 of each solver"""
    from pyro2_amd import device
    from pyro2_amd.pyro_sim import Pyro
    monkeypatch.setattr(device.Context, "_default", hip)
    monkeypatch.chdir(tmp_path)
    g = golden("comp_fv4_h5")
    p = Pyro(solver)
    p.initialize_problem("acoustic_pulse", inputs_file="inputs.acoustic_pulse",
                         inputs_dict={"gpu.fast_math": fast})
    p.run_sim()
    assert p.sim.n == int(g[solver + "_nsteps"]) == 160
    assert abs(p.sim.cc_data.t - float(g[solver + "_time"])) < 1e-12 and abs(p.sim.cc_data.t - 0.24) < 1e-12
    U = np.stack([p.get_var(nm).v() for nm in NAMES], axis=-1)
    gold = g[solver + "_gold"]
    scale = np.abs(gold).max(axis=(0, 1))
    err = (np.abs(U - gold) / scale).max(axis=(0, 1))
    print(solver, fast, err)
    assert err.max() <= 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["compressible_fv4", "compressible_sdc"])
def test_fv4_sdc_fourth_order_convergence(hip, tmp_path, monkeypatch, solver):
    """the acoustic pulse at 64^2, 128^2, 256^2 with dt halved with dx: observed L2 order of
    the density >= 3.7 (compressible_fv4/tests/convergence.txt records 3.97)"""
    from pyro2_amd import device
    from pyro2_amd.pyro_sim import Pyro
    monkeypatch.setattr(device.Context, "_default", hip)
    monkeypatch.chdir(tmp_path)
    rho = {}
    for n, dt in ((64, 3e-3), (128, 1.5e-3), (256, 7.5e-4)):
        p = Pyro(solver)
        p.initialize_problem("acoustic_pulse", inputs_file="inputs.acoustic_pulse",
                             inputs_dict={"mesh.nx": n, "mesh.ny": n, "driver.fix_dt": dt,
                                          "gpu.fast_math": 0})
        p.run_sim()
        rho[n] = np.array(p.get_var("density").v())

    def restrict(a):
        return 0.25 * (a[0::2, 0::2] + a[1::2, 0::2] + a[0::2, 1::2] + a[1::2, 1::2])

    e1 = np.sqrt(np.mean((restrict(rho[128]) - rho[64])**2))
    e2 = np.sqrt(np.mean((restrict(rho[256]) - rho[128])**2))
    order = np.log2(e1 / e2)
    print(solver, "L2 64-128", e1, "128-256", e2, "order", order)
    assert order >= 3.7


def test_fv4_refusals(api):
    """decomposition, SphericalPolar, well_balanced, non-square cells"""
    from pyro2_amd.pyro_sim import Pyro
    cases = [{"gpu.decompose": 1},
             {"mesh.grid_type": "SphericalPolar"},
             {"compressible.well_balanced": 1}]
    for extra in cases:
        p = Pyro("compressible_fv4")
        # (gpu.decompose = 1 with one process is refused by the driver already)
        with pytest.raises((SystemExit, RuntimeError)):
            p.initialize_problem("acoustic_pulse", inputs_file="inputs.acoustic_pulse",
                                 inputs_dict=dict({"mesh.nx": 16, "mesh.ny": 16}, **extra))
    p = Pyro("compressible_sdc")
    with pytest.raises(AssertionError, match="square"):
        p.initialize_problem("acoustic_pulse", inputs_file="inputs.acoustic_pulse",
                             inputs_dict={"mesh.nx": 16, "mesh.ny": 24})


@pytest.mark.parametrize("fast", [0, 1])
def test_fv4_invalid_state(api, golden, fast):
    """a negative density, and separately a NaN pressure, in an interior cell: ERR_STATE and k
    untouched; Pyro.single_step raises PyroHipError"""
    from pyro2_amd._lib import ERR_STATE, PyroHipError
    from pyro2_amd.pyro_sim import Pyro
    g = golden("comp_fv4_rhs")
    U0, bcs, meta = g["pulse_U"], g["pulse_bcs"], g["pulse_meta"]
    for bad in ("rho", "nan"):
        U = U0.copy()
        if bad == "rho":
            U[10, 12, 0] = -1.0
        else:
            U[10, 12, 1] = np.nan
        with pytest.raises(PyroHipError) as ei:
            _rhs(api, U, bcs, meta, fast)
        assert ei.value.code == ERR_STATE
    from pyro2_amd import device
    s = device.DeviceState(api, 32, 32, 4, [[str(b) for b in r] for r in bcs])
    U = U0.copy()
    U[10, 12, 0] = -1.0
    s.upload(U)
    k = device.DeviceState(api, 32, 32, 4, [["outflow"] * 4] * 4)
    k.upload(np.full((40, 40, 4), 7.0))
    P = device.make_comp_params(meta[0], meta[1], fast_math=fast, riemann="CGF")
    with pytest.raises(PyroHipError):
        s.comp_fv4_rhs(P, k, 0)
    assert np.all(k.download() == 7.0)
    p = Pyro("compressible_fv4")
    p.initialize_problem("acoustic_pulse", inputs_file="inputs.acoustic_pulse",
                         inputs_dict={"mesh.nx": 16, "mesh.ny": 16, "gpu.fast_math": fast})
    p.get_var("energy")[6, 7] = np.nan
    with pytest.raises(PyroHipError):
        p.single_step()


@pytest.mark.parametrize("solver", ["compressible_fv4", "compressible_sdc"])
def test_fv4_output_and_restart(api, tmp_path, solver):
    """an output file of an fv4 run is read back by io_pyro.read; a restart from it continues
    bit-identically to the uninterrupted run (no second from_centers)"""
    from pyro2_amd.pyro_sim import Pyro
    from pyro2_amd.util import io_pyro
    opts = {"mesh.nx": 16, "mesh.ny": 16, "driver.fix_dt": -1.0, "gpu.fast_math": 0}
    full = Pyro(solver)
    full.initialize_problem("acoustic_pulse", inputs_file="inputs.acoustic_pulse",
                            inputs_dict=dict(opts, **{"driver.max_steps": 4}))
    for _ in range(4):
        full.single_step()
    part = Pyro(solver)
    part.initialize_problem("acoustic_pulse", inputs_file="inputs.acoustic_pulse",
                            inputs_dict=dict(opts, **{"driver.max_steps": 2}))
    part.single_step()
    part.single_step()
    fname = str(tmp_path / "fv4_chk")
    part.sim.write(fname)
    chk = io_pyro.read(fname + ".h5")
    assert np.array_equal(np.array(chk.cc_data.get_var("density").v()),
                          np.array(part.get_var("density").v()))
    again = Pyro(solver)
    again.restart_problem(fname + ".h5", inputs_dict={"driver.max_steps": 4})
    again.single_step()
    again.single_step()
    for nm in NAMES:
        assert np.array_equal(np.array(again.get_var(nm).v()), np.array(full.get_var(nm).v())), nm
    assert again.sim.n == full.sim.n == 4
