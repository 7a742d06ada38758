"""advection_nonuniform (linear advection in a cell-by-cell velocity field) on the device against
runs of the reference (tools/gen_advnu_golden.py): the one-launch step of
csrc/advection_nonuniform.hip stage by stage, the several-steps call, short runs through the
driver, the reference's regression problem and its stored output file, the output files this
package writes, tracer particles, argument checks, and the reference's own unit test.

Tolerances.  The bit-faithful build (gpu.fast_math = 0: no FMA contraction, the reference's
operation order, a true division in the Courant number) is held to equality, ghost frame
included.  The contracted build is held to the project's advection tolerance, 1e-12 by
conftest.max_rel_err, for one step; for the 248 steps of the regression run to
max(10 x twin_dev, 1e-12), twin_dev being what a run of the reference with 1e-15 relative noise
on its velocities differs by from the clean one (advnu_regress.npz; measured figures: DESIGN)."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, max_rel_err
from pyro2_amd import _lib, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/pyro"
NAMES = ["x-velocity", "y-velocity", "x-shift", "y-shift", "density"]
IU, IV, IA = 0, 1, 4
NCASES = 7
SLOTTED = ((33, 36), (16, 19))


def _case(golden, k):
    g = golden("advnu_stages")
    assert int(g["ncases"]) == NCASES
    pre = f"c{k}_"
    m = g[pre + "meta"]
    c = {"nx": int(m[0]), "ny": int(m[1]), "ng": int(m[2]), "lim": int(m[3]), "dx": float(m[4]),
         "dy": float(m[5]), "cfl": float(m[6]), "bc": [[str(b) for b in row] for row in g[pre + "bc"]]}
    for key in ("Uin", "new", "a_x", "a_y", "F_x", "F_y"):
        c[key] = g[pre + key]
    c["dt"], c["dt_method"] = float(g[pre + "dt"]), float(g[pre + "dt_method"])
    return c


def _state(dev, c, planes=None):
    s = device.DeviceState(dev, c["nx"], c["ny"], c["ng"], c["bc"])
    s.upload(np.ascontiguousarray(np.moveaxis(c["Uin"] if planes is None else planes, 0, -1)))
    return s


def _planes(s):
    return np.ascontiguousarray(np.moveaxis(s.download(), -1, 0))


def _same(got, ref, what):
    d = np.abs(np.asarray(got) - np.asarray(ref)).max()
    print(f"{what}: max |diff| = {d:.3e}, max |ref| = {np.abs(ref).max():.3e}")
    assert np.array_equal(got, ref), (what, d)


@pytest.mark.parametrize("k", range(NCASES))
def test_stages_bit_for_bit(dev, golden, k):
    """one fill_BC_all + evolve() of the reference per case, from planes whose ghost cells hold
    junk (the step applies the boundary rules itself): uniform flow, the slotted rotation with
    its lines of v == 0 / u == 0, random-sign fields with 0.0 and -0.0 entries on grids of
    several tiles with ragged ends, v == 0 everywhere; limiter 0 / 1 / 2; periodic, outflow,
    walls in x, walls in y.  States, fluxes, the new density with its ghost frame and the time
    step equal the reference's, bit for bit."""
    c = _case(golden, k)
    ng, nx, ny = c["ng"], c["nx"], c["ny"]
    s = _state(dev, c)
    st = s.advnu_stages(IA, IU, IV, c["dx"], c["dy"], c["dt"], c["lim"])
    # where the update reads them (elsewhere the reference's scratch arrays hold zeros or
    # values built from them)
    fx = (slice(ng, ng + nx + 1), slice(ng, ng + ny))
    fy = (slice(ng, ng + nx), slice(ng, ng + ny + 1))
    _same(st[0][ng:ng + nx + 1, ng - 1:ng + ny + 1], c["a_x"][ng:ng + nx + 1, ng - 1:ng + ny + 1], "a_x")
    _same(st[1][ng - 1:ng + nx + 1, ng:ng + ny + 1], c["a_y"][ng - 1:ng + nx + 1, ng:ng + ny + 1], "a_y")
    _same(st[2][fx], c["F_x"][fx], "F_x")
    _same(st[3][fy], c["F_y"][fy], "F_y")
    _same(_planes(s), c["Uin"], "the state after the stage dump")
    s.advnu_step(IA, IU, IV, c["dx"], c["dy"], c["dt"], c["lim"])
    out = _planes(s)
    _same(out[IA], c["new"], "new density, ghost frame included")
    _same(out[:4], c["Uin"][:4], "velocities and shifts")
    # method_compute_timestep: over the whole array, after the driver's fill
    s.fill_bc(-1)
    dt = s.advnu_dt(IU, IV, c["dx"], c["dy"], c["cfl"])
    print("dt", dt, c["dt_method"])
    assert dt == c["dt_method"] and np.isfinite(dt)


@pytest.mark.parametrize("k", range(NCASES))
def test_stages_contracted_build(dev, golden, k):
    c = _case(golden, k)
    s = _state(dev, c)
    s.advnu_step(IA, IU, IV, c["dx"], c["dy"], c["dt"], c["lim"], fast_math=1)
    err = max_rel_err(_planes(s)[IA], c["new"])
    print(f"case {k}: contracted build, max_rel_err = {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("k", (1, 4))
@pytest.mark.parametrize("nsteps", (1, 2, 5))
def test_evolve_is_single_steps(dev, golden, k, nsteps):
    """pyrohip_advnu_evolve alternates between the state's plane and the work plane: odd and
    even step counts give, ghost frame included, what that many single steps give"""
    c = _case(golden, k)
    dts = [c["dt"] * f for f in (1.0, 0.7, 0.9, 0.35, 0.8)][:nsteps]
    one, many = _state(dev, c), _state(dev, c)
    for dt in dts:
        one.advnu_step(IA, IU, IV, c["dx"], c["dy"], dt, c["lim"])
    many.advnu_evolve(IA, IU, IV, c["dx"], c["dy"], dts, c["lim"])
    _same(_planes(many), _planes(one), f"{nsteps} steps in one call")
    assert not np.array_equal(_planes(many)[IA], c["Uin"][IA])


@pytest.fixture
def api(dev, tmp_path, monkeypatch):
    monkeypatch.setattr(device.Context, "_default", dev)
    monkeypatch.chdir(tmp_path)
    return dev


def _pyro(nx, ny, nsteps, extra=None, inputs_file=None):
    from pyro2_amd.pyro_sim import Pyro
    p = Pyro("advection_nonuniform")
    over = {"gpu.fast_math": 0}
    if nx:
        over.update({"mesh.nx": nx, "mesh.ny": ny, "driver.max_steps": nsteps})
    over.update(extra or {})
    p.initialize_problem("slotted", inputs_file=inputs_file, inputs_dict=over)
    return p


def _data(p):
    cc = p.sim.cc_data
    d = np.asarray(cc.data)
    return np.ascontiguousarray(np.stack([d[:, :, cc.names.index(n)] for n in NAMES]))


@pytest.mark.parametrize("batched", (True, False))
@pytest.mark.parametrize("r", range(2))
@pytest.mark.parametrize("nsteps", (5, 20))
def test_short_runs(api, golden, r, nsteps, batched):
    """5 and 20 steps of `slotted` through the driver, its batched path (evolve_many) and
    evolve() called singly: time and data equal the reference's, ghost cells included"""
    g = golden("advnu_runs")
    nx, ny = SLOTTED[r]
    p = _pyro(nx, ny, nsteps)
    assert p.sim.cc_data.names == NAMES
    if batched:
        assert p.sim.can_evolve_many()
        p.run_sim()
    else:
        while not p.sim.finished():
            p.single_step()
    assert p.sim.n == nsteps and p.sim.cc_data.t == float(g[f"r{r}_t{nsteps}"])
    _same(_data(p), g[f"r{r}_state{nsteps}"], f"{nx} x {ny}, {nsteps} steps")


def _reference_file(tmp_path):
    with gzip.open(os.path.join(GOLDEN, "slotted_0248.h5.gz"), "rb") as z:
        (tmp_path / "ref_slotted_0248.h5").write_bytes(z.read())
    return str(tmp_path / "ref_slotted_0248.h5")


def test_regression_slotted_0248(api, tmp_path, golden):
    """pyro/test.py's line for this solver: inputs.slotted to the end.  The bit-faithful build
    reproduces the reference's stored output file bit for bit; the contracted build stays
    within the reference's own sensitivity to 1e-15 noise on its velocities."""
    from pyro2_amd.util import h5pure
    p = _pyro(0, 0, 0)
    p.run_sim()
    assert p.sim.n == 248
    with h5pure.File(_reference_file(tmp_path)) as f:
        assert int(f.attrs["nsteps"]) == 248
        assert p.sim.cc_data.t == float(f.attrs["time"])
        stored = {n: np.array(f["state"][n]["data"][:, :]) for n in NAMES}
    for n in NAMES:
        _same(np.asarray(p.sim.cc_data.get_var(n).v()), stored[n], n)
    reg = golden("advnu_regress")
    assert int(reg["n"]) == 248 and int(reg["twin_n"]) == 248
    assert np.array_equal(reg["density"], stored["density"])      # the reference as it runs today
    q = _pyro(0, 0, 0, {"gpu.fast_math": 1})
    q.run_sim()
    bar = max(10.0 * float(reg["twin_dev"]), 1e-12)
    err = max_rel_err(np.asarray(q.sim.cc_data.get_var("density").v()), stored["density"])
    print(f"contracted build after 248 steps: max_rel_err = {err:.3e}, twin_dev = "
          f"{float(reg['twin_dev']):.3e}, bar = {bar:.3e}")
    assert q.sim.n == 248 and err <= bar


def test_output_file_and_restart(api, tmp_path):
    """the file the driver writes has the reference's groups, dataset names, order and
    attributes; io_pyro.read restores it and a restarted run continues bit for bit"""
    from pyro2_amd.advection_nonuniform import Simulation
    from pyro2_amd.pyro_sim import Pyro
    from pyro2_amd.util import h5pure, io_pyro
    p = _pyro(16, 19, 6, {"io.do_io": 1, "io.basename": "nu_", "io.n_out": 3, "io.dt_out": 1e33})
    p.run_sim()
    assert os.path.exists("nu_0003.h5") and os.path.exists("nu_0006.h5")
    with h5pure.File(_reference_file(tmp_path)) as ref, h5pure.File("nu_0003.h5") as f:
        assert set(ref) <= set(f)
        assert list(f["state"]) == list(ref["state"])
        for k in ("solver", "problem"):
            assert f.attrs[k] == ref.attrs[k] or f.attrs[k] == ref.attrs[k].decode()
        assert int(f.attrs["nsteps"]) == 3 and "time" in f.attrs
        assert set(ref["grid"].attrs) <= set(f["grid"].attrs)
        for n in ref["state"]:
            a, b = f["state"][n], ref["state"][n]
            assert list(a) == list(b) == ["data"]
            assert a["data"].shape == (16, 19) and a["data"].dtype == b["data"].dtype
            assert set(a.attrs) == set(b.attrs) == {"xlb", "xrb", "ylb", "yrb"}
            for k in a.attrs:
                assert a.attrs[k] == b.attrs[k]
    back = io_pyro.read("nu_0003.h5")
    assert isinstance(back, Simulation) and back.n == 3
    q = Pyro("advection_nonuniform")
    q.restart_problem("nu_0003.h5", inputs_dict={"io.do_io": 0})
    assert q.sim.n == 3
    for n in NAMES:
        assert np.array_equal(np.asarray(back.cc_data.get_var(n).v()), np.asarray(q.sim.cc_data.get_var(n).v()))
    q.run_sim()
    assert q.sim.n == 6 and q.sim.cc_data.t == p.sim.cc_data.t
    I = (slice(None), slice(4, -4), slice(4, -4))
    _same(_data(q)[I], _data(p)[I], "restarted run")


@pytest.mark.parametrize("batched", (True, False))
def test_particles(api, golden, batched):
    """tracer particles ride on the real velocity arrays: positions after 5 steps equal the
    reference's"""
    g = golden("advnu_runs")
    p = _pyro(33, 36, 5, {"particles.do_particles": 1, "particles.n_particles": 25})
    if batched:
        assert p.sim.can_evolve_many()
        p.run_sim()
    else:
        while not p.sim.finished():
            p.single_step()
    _same(p.sim.particles.get_init_positions(), g["part_init"], "initial positions")
    _same(p.sim.particles.get_positions(), g["part_pos5"], "positions after 5 steps")
    _same(_data(p), g["part_state5"], "data")


def test_argument_checks(dev, golden):
    """refusals come back as the argument error code; nothing is launched"""
    c = _case(golden, 0)
    s = _state(dev, c)
    before = _planes(s)

    def refused(call):
        with pytest.raises(_lib.PyroHipError) as e:
            call()
        assert e.value.code != 0
        return str(e.value)

    assert "limiter" in refused(lambda: s.advnu_step(IA, IU, IV, c["dx"], c["dy"], c["dt"], 3))
    assert "limiter" in refused(lambda: s.advnu_step(IA, IU, IV, c["dx"], c["dy"], c["dt"], -1))
    assert "dx" in refused(lambda: s.advnu_step(IA, IU, IV, 0.0, c["dy"], c["dt"], 2))
    assert "index" in refused(lambda: s.advnu_step(5, IU, IV, c["dx"], c["dy"], c["dt"], 2))
    assert "velocities" in refused(lambda: s.advnu_step(IU, IU, IV, c["dx"], c["dy"], c["dt"], 2))
    assert "limiter" in refused(lambda: s.advnu_evolve(IA, IU, IV, c["dx"], c["dy"], [c["dt"]] * 2, 7))
    assert np.array_equal(_planes(s), before)
    for ng in (3, 5):
        t = device.DeviceState(dev, 8, 8, ng, c["bc"])
        assert "ng = 4" in refused(lambda: t.advnu_step(IA, IU, IV, c["dx"], c["dy"], c["dt"], 2))
    for var in (IA, IU, IV):
        bc = [list(row) for row in c["bc"]]
        bc[var][3] = "moving_lid"
        t = device.DeviceState(dev, 8, 8, 4, bc)
        assert "boundaries only" in refused(lambda: t.advnu_step(IA, IU, IV, c["dx"], c["dy"], c["dt"], 2))
    # the code of an argument error, as the C header names it
    with pytest.raises(_lib.PyroHipError) as e:
        s.advnu_step(IA, IU, IV, c["dx"], c["dy"], c["dt"], 3)
    assert e.value.code == ERR_ARG


ERR_ARG = 10001


def test_solver_is_registered():
    import pyro
    from pyro2_amd import pyro_sim
    assert "advection_nonuniform" in pyro_sim.valid_solvers
    import pyro.advection_nonuniform.simulation as sim
    from pyro.advection_nonuniform.problems import test
    import pyro2_amd.advection_nonuniform.simulation as real
    assert sim is real and callable(test.init_data) and pyro.__name__ == "pyro"


PLUGIN = '''
import os, sys
ROOT = {root!r}
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu
from pyro2_amd import _lib, device
_lib.use_library(build_emu.LIB, allow_backends=("host-emu",))
device.Context._default = device.Context(0)
import matplotlib
matplotlib.use("Agg")
import pyro
assert os.path.realpath(pyro.__file__).startswith(os.path.realpath(ROOT))
'''


@pytest.mark.skipif(not os.path.exists(REF), reason="no reference checkout here")
def test_reference_unit_test_passes_on_the_alias_package(tmp_path):
    """the reference's own advection_nonuniform/tests/test_advection_nonuniform.py, unmodified,
    with `pyro` resolving to this repository's alias package (kernels on the HIP emulator)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    build_emu.build()
    (tmp_path / "ref_unit_plugin.py").write_text(PLUGIN.format(root=ROOT))
    f = os.path.join(REF, "advection_nonuniform/tests/test_advection_nonuniform.py")
    assert "pyro2_amd" not in open(f).read()
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path), ROOT]), MPLBACKEND="Agg",
               PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "ref_unit_plugin", "-p",
                        "no:cacheprovider", f"--rootdir={tmp_path}", f], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    assert "1 passed" in r.stdout, tail
