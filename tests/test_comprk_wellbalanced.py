"""compressible_rk with compressible.well_balanced = 1 (compressible_rk/fluxes.py:100-108, :139-148,
mesh/reconstruction.py:21-53) against runs of the reference, tests/golden/comp_rk_wb.npz
(tools/gen_comprk_wb_golden.py): ten small stratified atmospheres, the first stage of the first
step and three steps each, and the atmosphere at rest for twenty.

Tolerances.  The bit-faithful build (fast_math = 0) repeats the reference operation for
operation: bit for bit on the emulated backend, 10 x 1e-13 per step on the GPU, scaled per
variable, as test_device_compressible.test_compressible_rk.  The contracted build: 1e-10
element-wise, the project's tolerance for compressible; the reference's own answer to 1e-15
relative noise on the initial data (`twin_dev`) stays below 1.2e-13 in every case, and a path that
ignored the option would be off by `plain_dev` >= 1.3e-3.
"""
import numpy as np
import pytest

from conftest import comp_floors, elementwise_err, max_rel_err
from helpers import RK_TABLEAU, DtPolicy
from oracle import orc
from pyro2_amd import device
from pyro2_amd._lib import PyroHipError

TOL_EXACT = 1e-13
TOL_FAST = 1e-10
NCASES = 10
NAMES = ("density", "energy", "x-momentum", "y-momentum")
SIDES = ("mesh.xlboundary", "mesh.xrboundary", "mesh.ylboundary", "mesh.yrboundary")


class Case:
    def __init__(self, g, k):
        pre = self.pre = f"c{k}_"
        self.g = g
        self.meta = g[pre + "meta"]
        self.bcs = [str(b) for b in g[pre + "bc"]]
        self.method, self.riemann = str(g[pre + "method"]), str(g[pre + "riemann"])
        self.sp = g[pre + "sponge"]
        self.nx, self.ny, self.ng = int(self.meta[0]), int(self.meta[1]), int(self.meta[2])
        ng = self.ng
        self.I = (slice(ng, -ng), slice(ng, -ng))
        self.a, self.b = RK_TABLEAU[self.method]
        self.ns = len(self.b)

    def __getitem__(self, key):
        return self.g[self.pre + key]

    def params(self, **kw):
        nx, ny, ng, dx, dy, gamma, lim, flat, z0, z1, delta, cvisc, grav, cfl = self.meta
        solid = [int(b == "reflect") for b in self.bcs]
        kw.setdefault("well_balanced", 1)
        return device.make_comp_params(dx, dy, gamma=gamma, limiter=int(lim), use_flattening=int(flat), z0=z0,
                                       z1=z1, delta=delta, cvisc=cvisc, grav=grav, riemann=self.riemann,
                                       solid_xl=solid[0], solid_yl=solid[2],
                                       sponge=tuple(self.sp[1:]) if self.sp[0] else None, **kw), cfl

    def states(self, dev, n=2):
        vb = [list(r) for r in orc.comp_var_bcs(self.bcs)]
        out = [device.DeviceState(dev, self.nx, self.ny, self.ng, vb) for _ in range(n)]
        for t in out:
            if "hse" in self.bcs:
                t.set_user_bc(self.meta[5], self.meta[12], self.meta[4], None)
        kst = device.DeviceState(dev, self.nx, self.ny, self.ng, [["outflow"] * 4] * (4 * self.ns))
        return out + [kst]

    def inputs(self, **over):
        """the inputs of the recorded run"""
        m = self.meta
        d = {"mesh.nx": self.nx, "mesh.ny": self.ny, "compressible.limiter": int(m[6]),
             "compressible.use_flattening": int(m[7]), "compressible.grav": float(m[12]),
             "compressible.riemann": self.riemann, "compressible.temporal_method": self.method,
             "compressible.well_balanced": 1, "sponge.do_sponge": int(self.sp[0]), "driver.tmax": 1.e3,
             "driver.verbose": 0, "vis.dovis": 0, "io.do_io": 0}
        d.update(zip(SIDES, self.bcs))
        d.update(over)
        return d


def scaled_err(a, ref, I):
    """max over the interior of |a - ref| / per-variable max (at least 1e-3)"""
    scale = np.maximum(np.abs(ref[I]).max(axis=(0, 1)), 1e-3)
    return float((np.abs(a[I] - ref[I]) / scale).max())


def recorded_problem(ic):
    def init(my_data, rp):
        for n, name in enumerate(NAMES):
            my_data.get_var(name)[:, :] = ic[:, :, n]
    return init


def atmosphere_at_rest(my_data, rp):
    """the generator's atmosphere with amp 0: rho = 1 + 0.5 exp(-2 y), p from the discrete balance
    upward from p[:, 0] = 5 + |grav|"""
    g = my_data.grid
    gamma, grav = rp.get_param("eos.gamma"), rp.get_param("compressible.grav")
    rho = np.empty((g.qx, g.qy))
    rho[:, :] = (1.0 + 0.5 * np.exp(-2.0 * np.asarray(g.y)))[np.newaxis, :]
    p = np.empty((g.qx, g.qy))
    p[:, 0] = 5.0 + abs(grav)
    for j in range(1, g.qy):
        p[:, j] = p[:, j - 1] + 0.5 * g.dy * (rho[:, j - 1] + rho[:, j]) * grav
    my_data.get_var("density")[:, :] = rho
    my_data.get_var("x-momentum")[:, :] = 0.0
    my_data.get_var("y-momentum")[:, :] = 0.0
    my_data.get_var("energy")[:, :] = p / (gamma - 1.0)


def pyro_run(problem, inputs, nsteps):
    from pyro2_amd.pyro_sim import Pyro
    p = Pyro("compressible_rk")
    p.add_problem("atmosphere", problem, problem_params={})
    p.initialize_problem("atmosphere", inputs_dict=dict(inputs, **{"driver.max_steps": nsteps}))
    dts = []
    while not p.sim.finished():
        p.single_step()
        dts.append(p.sim.dt)
    assert len(dts) == nsteps
    return np.array(dts), np.array(p.sim.cc_data.data)


@pytest.mark.parametrize("k", range(NCASES))
def test_wb_rhs(dev, golden, k):
    """the right-hand side of the recorded stage start, and the y face pressures of the staged
    kernels against p +- 0.5 dy rho grav +- 0.5 ldy with ldy the plane the reference's
    well_balance() returned"""
    c = Case(golden("comp_rk_wb"), k)
    P, _ = c.params(fast_math=0)
    s, _, kst = c.states(dev)
    U0 = c["U0"]
    s.upload(U0)
    s.comp_rk_rhs(P, kst, 0)
    kd = kst.download()[:, :, :4]
    err = scaled_err(kd, c["k"], c.I)
    print("case", k, "k: scaled error", err)
    tol = 0.0 if dev.kind == "emu" else TOL_EXACT
    assert err <= tol * 10
    # y face states on R(1); a face pressure comes back out of the conserved state, with the
    # roundings of E = p / (gamma - 1) + kinetic energy (a few ulp of E <= 10 p here)
    ng, gamma, grav, dy = c.ng, c.meta[5], c.meta[12], c.meta[4]
    R1 = (slice(ng - 1, -(ng - 1)), slice(ng - 1, -(ng - 1)))
    rho = U0[..., 0]
    pr = (U0[..., 1] - 0.5 * (U0[..., 2]**2 + U0[..., 3]**2) / rho) * (gamma - 1.0)
    ldy = c["wb"]
    for name, sgn in (("YM", -1.0), ("YP", 1.0)):
        F = s.comp_stage(name)[R1]        # (the planes hold nothing outside R(1))
        pf = (F[..., 1] - 0.5 * (F[..., 2]**2 + F[..., 3]**2) / F[..., 0]) * (gamma - 1.0)
        want = (pr + sgn * (0.5 * dy * rho * grav) + sgn * 0.5 * ldy)[R1]
        e = float((np.abs(pf - want) / np.abs(want)).max())
        print("case", k, name, "face pressure: relative error", e)
        assert e <= 1e-12


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("k", range(NCASES))
def test_wb_runs(dev, golden, k, fast):
    """the recorded steps through the C ABI: fill, comp_rk_dt with the driver's policy, stages,
    lincomb"""
    c = Case(golden("comp_rk_wb"), k)
    P, cfl = c.params(fast_math=fast)
    s, y, kst = c.states(dev)
    a, b, ns = c.a, c.b, c.ns
    dts_ref, fin = c["dts"], c["final"]
    nsteps = len(dts_ref)
    tol = 0.0 if dev.kind == "emu" else TOL_EXACT
    f0, mx = c["drv"]
    s.upload(c["ic"])
    pol = DtPolicy(1.e30, f0, mx)
    for n in range(nsteps):
        s.fill_bc()
        dt = pol(s.comp_rk_dt(P, cfl))
        print("case", k, "fast", fast, "step", n, "dt / recorded - 1:", dt / dts_ref[n] - 1)
        if fast:
            assert abs(dt / dts_ref[n] - 1) <= TOL_FAST
        else:
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
    U = s.download()
    if fast:
        fl = comp_floors(fin[c.I], c.meta[5])
        errs = [elementwise_err(U[c.I][..., n], fin[c.I][..., n], fl[n]) for n in range(4)]
        print("case", k, "contracted: element-wise errors", errs)
        assert max(errs) <= TOL_FAST
    else:
        err = scaled_err(U, fin, c.I)
        print("case", k, "exact: scaled error", err)
        assert err <= tol * nsteps * 10


@pytest.mark.parametrize("k", [0, 6, 9])
def test_wb_pyro(dev, golden, k, tmp_path, monkeypatch):
    """the recorded runs through Pyro("compressible_rk"); gpu.kernel_set 2 takes the staged
    kernels like -1, since the option forces them: the same bits"""
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    c = Case(golden("comp_rk_wb"), k)
    dts_ref, fin = c["dts"], c["final"]
    nsteps = len(dts_ref)
    tol = 0.0 if dev.kind == "emu" else TOL_EXACT
    got = {}
    for kset in (-1, 2):
        dts, U = pyro_run(recorded_problem(c["ic"]), c.inputs(**{"gpu.kernel_set": kset, "gpu.fast_math": 0}),
                          nsteps)
        print("case", k, "kernel_set", kset, "dt error", max_rel_err(dts, dts_ref), "state error",
              scaled_err(U, fin, c.I))
        assert np.abs(dts / dts_ref - 1).max() <= max(tol * nsteps * 10, 1e-13)
        assert scaled_err(U, fin, c.I) <= tol * nsteps * 10
        got[kset] = (dts, U[c.I])
    assert np.array_equal(got[-1][0], got[2][0]) and np.array_equal(got[-1][1], got[2][1])


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("k", [0, 3])
def test_wb_equilibrium(dev, golden, k, fast, tmp_path, monkeypatch):
    """the atmosphere at rest for 20 steps: max |y-momentum| stays three decades below what the
    reference's plain scheme leaves (the reference's well-balanced scheme sits nine decades
    below that bound: this says that the balancing works, it is no parity check); the plain
    scheme of the device exceeds the bound"""
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    g = golden("comp_rk_wb")
    c = Case(g, k)
    bound = 1e-3 * float(g[f"rest{k}_plain"])
    res = {}
    for wb in (1, 0):
        _, U = pyro_run(atmosphere_at_rest, c.inputs(**{"compressible.well_balanced": wb, "gpu.fast_math": fast}),
                        20)
        res[wb] = float(np.abs(U[c.I][..., 3]).max())
    print("case", k, "fast", fast, "max |y-momentum|: well-balanced", res[1], "plain", res[0], "bound", bound,
          "reference", float(g[f"rest{k}_wb"]), float(g[f"rest{k}_plain"]))
    assert res[1] <= bound
    assert res[0] > bound


def test_wb_contract(dev, golden, capsys, tmp_path, monkeypatch):
    """the option is the staged right-hand side's alone: no one-call step, and every other entry
    point refuses a parameter block that sets it"""
    c = Case(golden("comp_rk_wb"), 5)     # reflecting walls, no sponge: the one-call step applies
    s, y, kst = c.states(dev)
    s.upload(c["U0"])
    kw = dict(kernel_set=2, march_rows=16, fast_math=0)
    P0, cfl = c.params(well_balanced=0, **kw)
    P1, _ = c.params(**kw)
    assert s.comp_rk_can_fuse(P0, kst, c.ns)
    assert not s.comp_rk_can_fuse(P1, kst, c.ns)
    calls = {"comp_rk_step": lambda: s.comp_rk_step(P1, kst, 1e-5, c.a, c.b),
             "comp_rk_evolve": lambda: s.comp_rk_evolve(P1, kst, c.a, c.b, cfl, DtPolicy(1.e30), 1),
             "comp_step": lambda: s.comp_step(P1, 1e-5),
             "comp_evolve": lambda: s.comp_evolve(P1, cfl, DtPolicy(1.e30), 1),
             "comp_fv4_rhs": lambda: s.comp_fv4_rhs(P1, kst, 0)}
    for name, call in calls.items():
        with pytest.raises(PyroHipError, match="well_balanced"):
            call()
    assert np.array_equal(s.download(), c["U0"]), "a refused call touched the state"
    P2, _ = c.params(**kw)
    P2.limiter = 2
    with pytest.raises(PyroHipError, match="limiter == 1"):
        s.comp_rk_rhs(P2, kst, 0)
    # the solvers
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    from pyro2_amd.pyro_sim import Pyro
    p = Pyro("compressible_rk")
    p.add_problem("atmosphere", atmosphere_at_rest, problem_params={})
    capsys.readouterr()
    with pytest.raises(SystemExit):
        p.initialize_problem("atmosphere", inputs_dict=c.inputs(**{"compressible.limiter": 2}))
    assert "well-balanced only works for limiter == 1" in capsys.readouterr().out
    for solver in ("compressible_fv4", "compressible_sdc"):
        p = Pyro(solver)
        with pytest.raises(SystemExit):
            p.initialize_problem("acoustic_pulse", inputs_file="inputs.acoustic_pulse",
                                 inputs_dict={"mesh.nx": 16, "mesh.ny": 16, "compressible.well_balanced": 1})
        assert "well_balanced" in capsys.readouterr().out


def test_wb_off_is_the_default(dev, golden):
    """well_balanced = 0 given explicitly: the bits of a parameter block that leaves the member alone"""
    c = Case(golden("comp_rk_wb"), 5)
    nx, ny, ng, dx, dy, gamma, lim, flat, z0, z1, delta, cvisc, grav, cfl = c.meta
    kw = dict(gamma=gamma, limiter=int(lim), use_flattening=int(flat), z0=z0, z1=z1, delta=delta,
              cvisc=cvisc, grav=grav, riemann=c.riemann, solid_xl=1, solid_yl=1)
    out = []
    for P in (device.make_comp_params(dx, dy, **kw), device.make_comp_params(dx, dy, well_balanced=0, **kw)):
        s, _, kst = c.states(dev)
        s.upload(c["U0"])
        s.comp_rk_rhs(P, kst, 0)
        out.append(kst.download()[:, :, :4][c.I])
    assert np.array_equal(out[0], out[1])
    # ... and they are not the well-balanced ones
    s, _, kst = c.states(dev)
    s.upload(c["U0"])
    s.comp_rk_rhs(c.params()[0], kst, 0)
    assert not np.array_equal(kst.download()[:, :, :4][c.I], out[0])
