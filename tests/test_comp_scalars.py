"""Passive scalars in the compressible CTU step (k_ctu_fused<.., NA>) and the
compressible_react solver.

Oracle: the reference itself, run with its two eigenvalue assignments on the slice [:ns]
(tools/gen_comp_scalars_golden.py; recorded in tests/golden/comp_scalars.npz), plus properties
that need no reference: the scalars never touch the gas, one scalar never touches the other, and
the transport is linear.

Tolerances.  Bit-faithful build (fast_math 0): np.array_equal on the emulated backend and on the
GPU.  Contracted build (fast_math 1): the project's compressible tolerance, 1e-10 element-wise
with the per-variable floors of conftest.comp_floors (the scalars take the density's floor: they
are partial densities); its dts equal the reference's where the driver's max_dt_change bounds
them (every step after the first) and agree to 1e-10 in the first."""
import types

import numpy as np
import pytest

import comp_scalars_cases as cs
from conftest import comp_floors, elementwise_err
from helpers import DtPolicy
from pyro2_amd import device
from pyro2_amd._lib import PyroHipError


def floors(ref, gamma=1.4):
    fl = comp_floors(ref[..., :4], gamma)
    return np.concatenate([fl, np.full(ref.shape[-1] - 4, fl[0])])


def assert_close(U, ref, fm, what):
    """bit-faithful build: equal bits; contracted build: 1e-10 element-wise"""
    worst = max(elementwise_err(U[..., n], ref[..., n], f) for n, f in enumerate(floors(ref)))
    print(what, "fast_math", fm, "equal", np.array_equal(U, ref), "element-wise error %.3e" % worst)
    if fm == 0:
        assert np.array_equal(U, ref), (what, np.argwhere(U != ref)[:5])
    else:
        assert worst <= cs.TOL_FAST, (what, worst)


def assert_dts(dts, ref, fm, what):
    print(what, "dts", list(dts), "reference", list(ref))
    if fm == 0:
        assert list(dts) == list(ref), what
    else:
        assert np.abs(np.array(dts) / np.array(ref) - 1.0).max() <= cs.TOL_FAST, what


# ---- golden parity --------------------------------------------------------------------------

@pytest.mark.parametrize("fm", [0, 1])
@pytest.mark.parametrize("k", range(cs.NCASES))
def test_golden_parity_c_abi(dev, golden, k, fm):
    """c0-c4 through pyrohip_comp_dt / pyrohip_comp_step: the dts and all 6 planes, ghost frame
    included (the step leaves the old state's filled ghost cells in the new array, as the
    reference's in-place update does), with the ghost fill as a call of its own and folded into
    the kernel (fuse_fill)"""
    c = cs.golden_case(golden("comp_scalars"), k)
    for fuse in (False, True):
        U, dts = cs.run(dev, c["ic"], c["meta"], c["bcs"], c["riemann"], drv=c["drv"], fast_math=fm,
                        fuse_fill=fuse)
        assert_dts(dts, c["dts"], fm, (k, fuse))
        assert_close(U, c["final"], fm, (k, "fuse_fill" if fuse else "filled"))


@pytest.mark.parametrize("k", cs.PROPERTY_CASES)
def test_golden_parity_one_scalar(dev, golden, k):
    """the recorded run with fuel alone (5 planes: the NA = 1 instance)"""
    g = golden("comp_scalars")
    c = cs.golden_case(g, k)
    for fm in (0, 1):
        U, dts = cs.run(dev, c["ic"][..., :5], c["meta"], c["bcs"], c["riemann"], drv=c["drv"], fast_math=fm)
        assert_dts(dts, c["dts"], fm, k)
        assert_close(U, g[f"c{k}_f1_final"], fm, (k, "fuel alone"))


def scalar_sim(extra):
    """what a user writes: compressible.Simulation with extra_vars"""
    from pyro2_amd import compressible

    class Sim(compressible.Simulation):
        def initialize(self, *, extra_vars=None, ng=4):
            super().initialize(extra_vars=list(extra), ng=ng)
    return Sim


def pyro_with_scalars(dev, monkeypatch, tmp_path, extra, problem, inputs, solver="compressible",
                      problem_name="recorded"):
    from pyro2_amd.pyro_sim import Pyro
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    p = Pyro(solver)
    if extra is not None:
        p.solver = types.SimpleNamespace(Simulation=scalar_sim(extra))
    if problem is not None:
        p.add_problem(problem_name, problem)
    d = {"driver.verbose": 0, "io.do_io": 0, "vis.dovis": 0}
    d.update(inputs)
    p.initialize_problem(problem_name, inputs_dict=d)
    return p


def case_inputs(c, fm):
    meta = c["meta"]
    d = {"mesh.nx": int(meta[0]), "mesh.ny": int(meta[1]), "eos.gamma": float(meta[5]),
         "compressible.limiter": int(meta[6]), "compressible.use_flattening": int(meta[7]),
         "compressible.cvisc": float(meta[11]), "compressible.grav": float(meta[12]),
         "driver.cfl": float(meta[13]), "compressible.riemann": c["riemann"], "driver.tmax": 1.e3,
         "driver.max_steps": 1000000, "gpu.fast_math": fm}
    d.update(zip(("mesh.xlboundary", "mesh.xrboundary", "mesh.ylboundary", "mesh.yrboundary"), c["bcs"]))
    return d


@pytest.mark.parametrize("fm", [0, 1])
@pytest.mark.parametrize("k", range(cs.NCASES))
def test_golden_parity_pyro(dev, golden, k, fm, monkeypatch, tmp_path):
    """the same runs through Pyro.single_step with a user's Simulation subclass that passes
    extra_vars: registration order, boundary types, the driver's dt policy, the lazy ghost fill"""
    c = cs.golden_case(golden("comp_scalars"), k)

    def recorded(my_data, rp):
        for n, name in enumerate(cs.NAMES):
            my_data.get_var(name)[:, :] = c["ic"][:, :, n]
    p = pyro_with_scalars(dev, monkeypatch, tmp_path, ("fuel", "ash"), recorded, case_inputs(c, fm))
    sim = p.sim
    assert sim.cc_data.names == cs.NAMES and sim.ivars.naux == 2 and sim.ivars.irhox == 4
    assert not sim.can_evolve_many()
    dts = []
    for _ in range(cs.NSTEPS):
        p.single_step()
        dts.append(sim.dt)
    assert_dts(dts, c["dts"], fm, k)
    assert_close(np.array(sim.cc_data.data), c["final"], fm, (k, "Pyro"))
    # the primitive variables carry the mass fractions behind rho, u, v, p
    q = sim.cc_data.get_var("primitive")
    assert len(q) == 6
    assert np.array_equal(np.asarray(q[4]), c_div(sim, "fuel")) and np.array_equal(np.asarray(q[5]), c_div(sim, "ash"))


def c_div(sim, name):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(sim.cc_data.get_var(name)) / np.asarray(sim.cc_data.get_var("density"))


def test_run_sim_with_scalars(dev, golden, monkeypatch, tmp_path):
    """run_sim: the loop falls back to single steps (no device-side stepping with scalars) and
    ends where the single steps do"""
    c = cs.golden_case(golden("comp_scalars"), 0)

    def recorded(my_data, rp):
        for n, name in enumerate(cs.NAMES):
            my_data.get_var(name)[:, :] = c["ic"][:, :, n]
    d = case_inputs(c, 0)
    d["driver.max_steps"] = cs.NSTEPS
    p = pyro_with_scalars(dev, monkeypatch, tmp_path, ("fuel", "ash"), recorded, d)
    p.run_sim()
    assert p.sim.n == cs.NSTEPS
    assert np.array_equal(np.array(p.sim.cc_data.data)[4:-4, 4:-4], c["final"][4:-4, 4:-4])


# ---- properties -----------------------------------------------------------------------------

_PROPERTY_RUNS = {}


def property_runs(dev, golden, label, fm):
    """the four runs of a shape, once per backend and build: the gas alone, fuel and ash, fuel
    alone, fuel halved"""
    key = (dev.kind, label, fm)
    if key not in _PROPERTY_RUNS:
        ic, meta, bcs, riemann, drv = cs.property_case(golden("comp_scalars"), label)
        half = ic.copy()
        half[..., 4] *= 0.5
        kw = dict(riemann=riemann, drv=drv, fast_math=fm, kernel_set=1)
        _PROPERTY_RUNS[key] = {name: cs.run(dev, a, meta, bcs, **kw) for name, a in
                               (("gas", ic[..., :4]), ("both", ic), ("fuel", ic[..., :5]), ("half", half))}
    return _PROPERTY_RUNS[key]


def check_properties(dev, golden, label, fm):
    r = property_runs(dev, golden, label, fm)
    (Ug, dg), Ub, Uf, Uh = r["gas"], r["both"][0], r["fuel"][0], r["half"][0]
    ng = 4
    I = (slice(ng, -ng), slice(ng, -ng))
    assert np.abs(Ub[I][..., 4] - Ub[I][..., 4].mean()).max() > 1e-3     # (something to transport)
    # 1. the scalars never touch the gas: hydro planes and dt of the 4-variable run
    for name, (U, dts) in (("both", r["both"]), ("fuel", r["fuel"]), ("half", r["half"])):
        same = np.array_equal(U[..., :4], Ug) and dts == dg
        worst = max(elementwise_err(U[..., n], Ug[..., n], f) for n, f in enumerate(comp_floors(Ug)))
        print(label, "fast_math", fm, name, "hydro planes and dt bit-identical:", same, "error %.3e" % worst)
        if fm == 0:
            assert same, (label, name)
        else:
            # contracted build: the 4-variable run takes other instances of the kernel (NA = 0,
            # with the default reconstruction as compile-time constants), in which the compiler is
            # free to contract differently
            assert worst <= cs.TOL_FAST and np.abs(np.array(dts) / np.array(dg) - 1).max() <= cs.TOL_FAST
    # 2. one scalar never touches the other
    assert np.array_equal(Uf[..., 4], Ub[..., 4]), (label, fm, np.abs(Uf[..., 4] - Ub[..., 4]).max())
    # 3. the transport is linear: halved data, halved plane, exactly
    assert np.array_equal(Uh[..., 4], 0.5 * Ub[..., 4]), (label, fm)
    assert np.array_equal(Uh[..., 5], Ub[..., 5]), (label, fm)


@pytest.mark.parametrize("fm", [0, 1])
@pytest.mark.parametrize("label", [c[0] for c in cs.PROPERTY_SHAPES if not c[3]])
def test_properties(dev, golden, label, fm):
    check_properties(dev, golden, label, fm)


@pytest.mark.gpu
@pytest.mark.parametrize("fm", [0, 1])
@pytest.mark.parametrize("label", [c[0] for c in cs.PROPERTY_SHAPES if c[3]])
def test_properties_many_tiles(hip, golden, label, fm):
    """112 x 240: 8 x 8 tiles, the XCD renumbering of the tile walk is active; 127 x 250: 90
    ragged tiles, identity walk"""
    check_properties(hip, golden, label, fm)


# ---- refusals -------------------------------------------------------------------------------

def refused(capsys, fn, *words):
    with pytest.raises(SystemExit):
        fn()
    text = capsys.readouterr().out
    assert "passive scalars" in text, text
    for w in words:
        assert w in text, (w, text)


REFUSED_INPUTS = [
    ("cgf", {"compressible.riemann": "CGF"}, "compressible.riemann"),
    ("spherical", {"mesh.grid_type": "SphericalPolar", "compressible.riemann": "CGF", "mesh.xmin": 0.1,
                   "mesh.ymin": 0.5, "mesh.ymax": 2.0}, "compressible.riemann"),
    ("spherical_hllc", {"mesh.grid_type": "SphericalPolar", "mesh.xmin": 0.1, "mesh.ymin": 0.5, "mesh.ymax": 2.0},
     "SphericalPolar"),
    ("decompose", {"gpu.decompose": 1}, "gpu.decompose"),
    ("hse", {"mesh.ylboundary": "hse", "mesh.yrboundary": "hse", "compressible.grav": -1.0}, "hse"),
    ("ambient", {"mesh.yrboundary": "ambient"}, "ambient"),
    ("ramp", {"mesh.ylboundary": "ramp"}, "ramp"),
    ("sponge", {"sponge.do_sponge": 1}, "sponge.do_sponge"),
    ("kernel_set_0", {"gpu.kernel_set": 0}, "gpu.kernel_set"),
    ("kernel_set_2", {"gpu.kernel_set": 2}, "gpu.kernel_set"),
]


@pytest.mark.parametrize("what, inputs, word", REFUSED_INPUTS, ids=[r[0] for r in REFUSED_INPUTS])
def test_refused_option(dev, monkeypatch, tmp_path, capsys, what, inputs, word):
    d = {"mesh.nx": 8, "mesh.ny": 8}
    d.update(inputs)
    if what == "decompose":      # (a decomposition in force: what a launcher's ranks install)
        from pyro2_amd import decomp
        monkeypatch.setattr(decomp, "active_decomposition",
                            lambda rp=None: types.SimpleNamespace(rank=0, nranks=2))
    refused(capsys, lambda: pyro_with_scalars(dev, monkeypatch, tmp_path, ("fuel",), None, d,
                                              problem_name="sedov"), word)


def test_refused_three_scalars(dev, monkeypatch, tmp_path, capsys):
    refused(capsys, lambda: pyro_with_scalars(dev, monkeypatch, tmp_path, ("a", "b", "c"), None,
                                              {"mesh.nx": 8, "mesh.ny": 8}, problem_name="sedov"), "at most two")


@pytest.mark.parametrize("host", [0, 1])
def test_refused_problem_source(dev, monkeypatch, tmp_path, capsys, host):
    """a heating profile (problem `heating`) and, with gpu.host_source, the same source evaluated
    on the host"""
    refused(capsys, lambda: pyro_with_scalars(dev, monkeypatch, tmp_path, ("fuel",), None,
                                              {"mesh.nx": 8, "mesh.ny": 8, "gpu.host_source": host},
                                              problem_name="heating"), "source")


@pytest.mark.parametrize("solver", ["compressible_rk", "compressible_fv4", "compressible_sdc"])
def test_refused_method_of_lines_solvers(dev, monkeypatch, tmp_path, capsys, solver):
    """nothing moved: extra_vars still fail in initialize there"""
    from pyro2_amd.pyro_sim import Pyro
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    p = Pyro(solver)
    base = p.solver.Simulation

    class Sim(base):
        def initialize(self, *, extra_vars=None, ng=4):
            super().initialize(extra_vars=["fuel"], ng=ng)
    p.solver = types.SimpleNamespace(Simulation=Sim)
    refused(capsys, lambda: p.initialize_problem("sedov", inputs_dict={"mesh.nx": 8, "mesh.ny": 8,
                                                                      "driver.verbose": 0, "io.do_io": 0}),
            solver, "extra_vars")


def six_plane_state(dev, bcs=("outflow",) * 4, n=16):
    U, meta = cs.rough_state(n, n, 11)
    s = cs.state(dev, n, n, list(bcs), 6)
    s.upload(U)
    s.fill_bc()
    return s, meta


def lib_refuses(fn, *words):
    with pytest.raises(PyroHipError) as e:
        fn()
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_c_abi_refusals_of_the_step(dev):
    """pyrohip_comp_step with 6 planes: what the scalars exclude, by the message"""
    s, meta = six_plane_state(dev)
    bcs = ["outflow"] * 4
    for kw, word in ((dict(riemann="CGF"), "CGF"), (dict(kernel_set=0), "kernel_set"),
                     (dict(kernel_set=2), "kernel_set"), (dict(sponge=(1e-2, 1e-3, 1e-2)), "sponge")):
        P, _ = cs.params(meta, bcs, **kw)
        lib_refuses(lambda: s.comp_step(P, 1e-4), "passive scalars", word)
    P, _ = cs.params(meta, bcs)
    s7 = cs.state(dev, 16, 16, bcs, 7)
    lib_refuses(lambda: s7.comp_step(P, 1e-4), "at most 2 passive scalars")
    lib_refuses(lambda: s7.comp_dt(P, 0.8), "at most 2 passive scalars")
    s.comp_step(P, 1e-4)           # ... and what is carried still steps
    assert s.comp_dt_is_cached()


def test_c_abi_other_entry_points_keep_four_planes(dev):
    """a 6-plane state is still refused by pyrohip_comp_evolve, pyrohip_comp_rk_*,
    pyrohip_comp_fv4_rhs and the swe and burgers entry points"""
    s, meta = six_plane_state(dev)
    bcs = ["outflow"] * 4
    P, cfl = cs.params(meta, bcs)
    k = cs.state(dev, 16, 16, bcs, 16)
    four = "must have 4 variables"
    lib_refuses(lambda: s.comp_evolve(P, cfl, DtPolicy(1.0), 2), four, "passive scalars")
    lib_refuses(lambda: s.comp_rk_rhs(P, k, 0), four)
    lib_refuses(lambda: s.comp_rk_dt(P, cfl), four)
    a, b = [[0.0, 0.0], [0.5, 0.0]], [0.0, 1.0]
    lib_refuses(lambda: s.comp_rk_step(P, k, 1e-4, a, b), four)
    lib_refuses(lambda: s.comp_rk_evolve(P, k, a, b, cfl, DtPolicy(1.0), 2), four)
    lib_refuses(lambda: s.comp_fv4_rhs(P, k, 0), four)
    lib_refuses(lambda: s.comp_source_correct(P, 1e-4), four)
    lib_refuses(lambda: s.swe_dt(1.0 / 16, 1.0 / 16, 1.0, 0.8), "swe state must have 4 variables")
    lib_refuses(lambda: s.swe_step(1.0 / 16, 1.0 / 16, 1.0, 2, "HLLC", 1e-4), "swe state must have 4 variables")
    lib_refuses(lambda: s.bg_step1(0, 1, 1.0 / 16, 1.0 / 16, 1e-4, 2))


# ---- compressible_react ---------------------------------------------------------------------

def react(dev, monkeypatch, tmp_path, problem, inputs):
    from pyro2_amd.pyro_sim import Pyro
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    p = Pyro("compressible_react")
    d = {"driver.verbose": 0, "io.do_io": 0, "vis.dovis": 0}
    d.update(inputs)
    p.initialize_problem(problem, inputs_dict=d)
    return p


def test_react_initial_conditions(dev, golden, monkeypatch, tmp_path, capsys):
    """flame (32 x 32) and rt (16 x 48) as the reference's init_data leaves them; rt's shipped hse
    sides are refused with scalars, reflecting ones step"""
    g = golden("comp_scalars")
    p = react(dev, monkeypatch, tmp_path, "flame", {"mesh.nx": 32, "mesh.ny": 32})
    assert p.sim.cc_data.names == cs.NAMES
    assert p.rp.get_param("compressible.riemann") == "HLLC"
    assert np.array_equal(np.array(p.sim.cc_data.data), g["react_flame_ic"])
    walls = {"mesh.nx": 16, "mesh.ny": 48, "mesh.ylboundary": "reflect", "mesh.yrboundary": "reflect"}
    p = react(dev, monkeypatch, tmp_path, "rt", walls)
    assert np.array_equal(np.array(p.sim.cc_data.data), g["react_rt_ic"], equal_nan=True)
    p.single_step()
    A = np.array(p.sim.cc_data.data)[4:-4, 4:-4]
    assert np.all(np.isfinite(A)) and p.sim.n == 1
    refused(capsys, lambda: react(dev, monkeypatch, tmp_path, "rt", {"mesh.nx": 16, "mesh.ny": 48}), "hse")


@pytest.mark.parametrize("fm", [0, 1])
def test_react_flame_is_the_blast_of_compressible(dev, monkeypatch, tmp_path, fm):
    """4 steps of flame at 32^2: fuel = ash = 0 and the hydro planes of the compressible solver --
    bit for bit from the same initial data (the flame module's, which sums its 16 sub-samples one
    after the other), and within 1e-12 of the `sedov` problem with r_init = 0.1, whose initial
    energy differs from flame's by one unit in the last place (2.3e-16 relative) in 16 cells: the
    count-then-multiply sum of sedov.py against the running sum"""
    from pyro2_amd.compressible_react.problems import flame
    size = {"mesh.nx": 32, "mesh.ny": 32, "gpu.fast_math": fm, "gpu.kernel_set": 1}
    p = react(dev, monkeypatch, tmp_path, "flame", size)
    q = pyro_with_scalars(dev, monkeypatch, tmp_path, None, flame.init_data, size, problem_name="flame")
    s = pyro_with_scalars(dev, monkeypatch, tmp_path, None, None, dict(size, **{"sedov.r_init": 0.1}),
                          problem_name="sedov")
    for _ in range(4):
        for run in (p, q, s):
            run.single_step()
    A, B, C = (np.array(r.sim.cc_data.data) for r in (p, q, s))
    assert p.sim.n == 4 and p.sim.cc_data.t == q.sim.cc_data.t
    assert np.all(A[..., 4:] == 0.0)
    worst = max(elementwise_err(A[..., n], B[..., n], f) for n, f in enumerate(comp_floors(B)))
    print("fast_math", fm, "flame vs compressible: equal", np.array_equal(A[..., :4], B), "error %.3e" % worst)
    if fm == 0:
        assert np.array_equal(A[..., :4], B)
    else:
        assert worst <= cs.TOL_FAST
    scale = np.abs(C).max(axis=(0, 1))
    assert (np.abs(A[..., :4] - C) / scale).max() <= (1e-12 if fm == 0 else cs.TOL_FAST)


@pytest.mark.parametrize("flag", [0, 1])
def test_react_tracer_quirk(dev, monkeypatch, tmp_path, flag):
    """the particles advance dt/2, dt (inside the hydro step) and dt/2 per step: 2 dt.  Against
    the host particle path driven by hand in that order on the states of a compressible run, for
    the device path (gpu.device_particles = 1) and the host path"""
    from pyro2_amd.compressible_react.problems import flame
    size = {"mesh.nx": 32, "mesh.ny": 32, "gpu.fast_math": 0, "particles.do_particles": 1,
            "particles.n_particles": 64, "particles.particle_generator": "grid",
            "gpu.device_particles": flag}
    p = react(dev, monkeypatch, tmp_path, "flame", size)
    q = pyro_with_scalars(dev, monkeypatch, tmp_path, None, flame.init_data,
                          dict(size, **{"gpu.device_particles": 0, "particles.do_particles": 0}),
                          problem_name="flame")
    from pyro2_amd.particles import particles
    ref = particles.Particles(q.sim.cc_data, p.sim.particles.bc, 64, "grid")

    def vel(sim):
        u, v = sim.cc_data.get_var_readonly("velocity")
        return u, v
    for _ in range(3):
        p.single_step()
        # the same step by hand: dt/2 on the old state, the hydro step, dt on the new state, dt/2
        q.sim.cc_data.fill_BC_all()
        q.sim.compute_timestep()
        dt = q.sim.dt
        ref.update_particles(dt / 2, *vel(q.sim))
        q.sim.evolve()
        ref.update_particles(dt, *vel(q.sim))
        ref.update_particles(dt / 2, *vel(q.sim))
        assert p.sim.dt == dt
    got, want = p.sim.particles.get_positions(), ref.get_positions()
    moved = np.abs(want - ref.get_init_positions()).max()
    err = np.abs(got - want).max()
    print("device_particles", flag, "moved", moved, "difference", err)
    assert moved > 1e-6
    # host path: the same arithmetic in the same order; device path: the project's bound for
    # tracer positions against the host path (tests/test_particles_device.py: round-off of one
    # interpolation per step)
    assert err <= (0.0 if flag == 0 else 1e-13)


def test_react_write_and_restart_round_trip(dev, monkeypatch, tmp_path):
    """an 8 x 8 file of six variables: read back equal, and a restarted run continues bit for bit"""
    from pyro2_amd.pyro_sim import Pyro
    from pyro2_amd.util import io_pyro
    size = {"mesh.nx": 8, "mesh.ny": 8, "gpu.fast_math": 0, "driver.max_steps": 4}

    def seeded(p):
        cc = p.sim.cc_data
        rng = np.random.default_rng(5)
        rho = np.array(cc.get_var("density"))
        cc.get_var("fuel")[:, :] = rho * rng.random(rho.shape)
        cc.get_var("ash")[:, :] = rho - np.array(cc.get_var("fuel"))
        return p
    p = seeded(react(dev, monkeypatch, tmp_path, "flame", size))
    for _ in range(2):
        p.single_step()
    p.sim.write("six")
    back = io_pyro.read("six")
    assert back.cc_data.names == cs.NAMES
    I = (slice(4, -4), slice(4, -4))
    assert np.array_equal(np.array(back.cc_data.data)[I], np.array(p.sim.cc_data.data)[I])
    assert np.abs(np.array(back.cc_data.data)[I][..., 4]).max() > 0
    r = Pyro("compressible_react")
    r.restart_problem("six", inputs_dict={"driver.verbose": 0, "io.do_io": 0})
    for _ in range(2):
        p.single_step()
        r.single_step()
    assert r.sim.n == p.sim.n == 4 and r.sim.cc_data.t == p.sim.cc_data.t
    assert np.array_equal(np.array(r.sim.cc_data.data)[I], np.array(p.sim.cc_data.data)[I])


def test_react_command_line_run(dev, monkeypatch, tmp_path):
    """`pyro_sim compressible_react flame inputs.flame` runs to tmax (here: a small grid and an
    early tmax) through run_sim"""
    p = react(dev, monkeypatch, tmp_path, "flame", {"mesh.nx": 16, "mesh.ny": 16, "driver.tmax": 2.e-3})
    p.run_sim()
    assert p.sim.cc_data.t == 2.e-3 and p.sim.n >= 3
    assert np.all(np.isfinite(np.array(p.sim.cc_data.data)[4:-4, 4:-4]))


# ---- nothing moved --------------------------------------------------------------------------

def test_four_variable_sedov_unchanged(dev, golden):
    """Sedov 64^2, 4 steps, the library's kernel choice, bit-faithful build: the tile kernel, one
    launch per step, and the bits recorded on the parent commit (a 16 x 16 window around the
    blast, recorded on the emulated backend; the GPU's bit-faithful build gives the same bits)"""
    from sedov_ic import sedov_ic
    g = golden("comp_scalars")
    U, meta, bcs = sedov_ic(64)
    P, cfl = cs.params(meta, bcs, kernel_set=-1, fast_math=0)
    s = cs.state(dev, 64, 64, bcs, 4)
    s.upload(U)
    pol, dts = DtPolicy(1.e30), []
    dev.prof_enable(True)
    try:
        dev.prof_report()
        for _ in range(4):
            s.fill_bc()
            dt = pol(s.comp_dt(P, cfl))
            s.comp_step(P, dt)
            pol.advance(dt)
            dts.append(dt)
        launches = {name: n for name, (n, _) in dev.prof_report().items()}
    finally:
        dev.prof_enable(False)
    assert launches.get("k_ctu_fused") == 4 and "k_ctu_wave" not in launches, launches
    W = s.download()[4 + 24:4 + 40, 4 + 24:4 + 40]
    ref = g["sedov64_window"]
    err = (np.abs(W - ref) / np.abs(ref).max(axis=(0, 1))).max()
    print("sedov 64^2 window: equal", np.array_equal(W, ref), "error %.3e" % err, "dts", dts)
    assert dts == list(g["sedov64_dts"]) and np.array_equal(W, ref)
