"""Generate tests/golden/advnu_*.npz by RUNNING THE REFERENCE's advection_nonuniform solver
(test infrastructure, build container only):

    cd /tmp && MPLBACKEND=Agg \\
      PYTHONPATH=<repo>/oracle/shim:<reference checkout> \\
      python3 <repo>/tools/gen_advnu_golden.py [stages] [runs] [regress] [h5]

The shim of oracle/ replaces numba.njit by the identity.  Nothing of the reference is copied:
its solver is run and its inputs / outputs stored.  The intermediates of unsplit_fluxes (a_x,
a_y are locals of it) are read from its frame when it returns, by a profile hook set around
evolve().
  advnu_stages.npz  one fill_BC_all + evolve() per case: the five planes before the fill (ghost
                    cells hold junk: the step under test has to apply the boundary rules), a_x,
                    a_y, F_x, F_y, the new density (its ghost frame is the fill of the old one),
                    dt of method_compute_timestep and of the driver's policy
  advnu_runs.npz    5 and 20 steps of `slotted` through Pyro(...).run_sim() at 33 x 36 and
                    16 x 19, and 5 steps with tracer particles
  advnu_regress.npz the regression run (inputs.slotted to the end: step count, time, density)
                    and its twin with 1e-15 relative noise on the velocities: `twin_dev`, the
                    twin's density deviation (the yardstick of the contracted build)
  slotted_0248.h5.gz  the reference's regression file, gzipped (an input of the regression test)

The reference imports h5py at import time (util/io_pyro.py); without h5py a stub module stands
in for it.
"""
import gzip
import os
import sys
import tempfile
import types

import numpy as np

try:
    import h5py  # noqa: F401
except ImportError:
    sys.modules["h5py"] = types.ModuleType("h5py")

os.chdir(tempfile.mkdtemp())   # Pyro writes inputs.auto into cwd

import pyro.advection_nonuniform.advective_fluxes as flx      # noqa: E402
from pyro.advection_nonuniform.problems import slotted         # noqa: E402
from pyro.pyro_sim import Pyro                                 # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
REF = os.path.dirname(os.path.abspath(sys.modules["pyro"].__file__))
NAMES = ["x-velocity", "y-velocity", "x-shift", "y-shift", "density"]
POLICY = {"driver.init_tstep_factor": 1.0, "driver.max_dt_change": 1.e33, "driver.tmax": 1.e3,
          "slotted.omega": 0.5, "slotted.offset": 0.25}
PERIODIC = {k: "periodic" for k in ("mesh.xlboundary", "mesh.xrboundary", "mesh.ylboundary", "mesh.yrboundary")}
OUTFLOW = {k: "outflow" for k in PERIODIC}
WALLS_X = {"mesh.xlboundary": "reflect", "mesh.xrboundary": "reflect",
           "mesh.ylboundary": "outflow", "mesh.yrboundary": "outflow"}
WALLS_Y = {"mesh.xlboundary": "outflow", "mesh.xrboundary": "outflow",
           "mesh.ylboundary": "reflect", "mesh.yrboundary": "reflect"}


def save(name, **kw):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **kw)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def planes(cc):
    d = np.array(cc.data)
    return np.ascontiguousarray(np.stack([d[:, :, cc.names.index(n)] for n in NAMES]))


def max_rel_err(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---- problems: every one fills the WHOLE arrays, ghost cells included (junk there) ----------

def _rough(my_data, rng):
    """random structure on top of the density, everywhere: the cells next to the ghost frame
    matter to the update"""
    dens = my_data.get_var("density")
    dens[:, :] = dens + rng.random(dens.shape)


def prob_rotation(seed):
    def init(my_data, rp):
        slotted.init_data(my_data, rp)
        _rough(my_data, np.random.default_rng(seed))
    return init


def prob_uniform(seed):
    def init(my_data, rp):
        slotted.init_data(my_data, rp)
        _rough(my_data, np.random.default_rng(seed))
        my_data.get_var("x-velocity")[:, :] = 1.0
        my_data.get_var("y-velocity")[:, :] = 1.0
    return init


def prob_random(seed):
    """velocities of random sign and size with exact 0.0 and -0.0 entries"""
    def init(my_data, rp):
        rng = np.random.default_rng(seed)
        slotted.init_data(my_data, rp)
        _rough(my_data, rng)
        for name in ("x-velocity", "y-velocity"):
            w = my_data.get_var(name)
            w[:, :] = 2.0 * rng.random(w.shape) - 1.0
            pick = rng.random(w.shape)
            w[pick < 0.04] = 0.0
            w[pick < 0.02] = -0.0
    return init


def prob_no_v(seed):
    def init(my_data, rp):
        slotted.init_data(my_data, rp)
        _rough(my_data, np.random.default_rng(seed))
        my_data.get_var("y-velocity")[:, :] = 0.0
    return init


def prob_noisy(noise, seed=11):
    def init(my_data, rp):
        slotted.init_data(my_data, rp)
        rng = np.random.default_rng(seed)
        for name in ("x-velocity", "y-velocity"):
            w = my_data.get_var(name)
            w[:, :] = w * (1.0 + noise * (2.0 * rng.random(w.shape) - 1.0))
    return init


def make(init, extra):
    p = Pyro("advection_nonuniform")
    p.add_problem("generated", init, problem_params=dict(slotted.PROBLEM_PARAMS))
    p.initialize_problem("generated", inputs_dict=extra)
    return p


def captured_evolve(sim):
    rec = {}
    code = flx.unsplit_fluxes.__code__

    def hook(frame, event, arg):
        if event == "return" and frame.f_code is code:
            for k in ("a_x", "a_y", "F_x", "F_y"):
                rec[k] = np.array(frame.f_locals[k])
    sys.setprofile(hook)
    try:
        sim.evolve()
    finally:
        sys.setprofile(None)
    return rec


def gen_stages():
    cases = [(8, 8, prob_uniform(1), 2, PERIODIC),
             (33, 36, prob_rotation(2), 2, PERIODIC),
             (16, 19, prob_rotation(3), 0, WALLS_X),
             (19, 150, prob_random(4), 2, OUTFLOW),
             (150, 19, prob_random(5), 1, WALLS_X),
             (24, 24, prob_no_v(6), 1, PERIODIC),
             (19, 150, prob_random(7), 2, WALLS_Y)]
    out = {"ncases": len(cases)}
    for k, (nx, ny, init, lim, sides) in enumerate(cases):
        p = make(init, dict(POLICY, **sides, **{"mesh.nx": nx, "mesh.ny": ny, "advection.limiter": lim}))
        sim = p.sim
        pre = f"c{k}_"
        out[pre + "Uin"] = planes(sim.cc_data)
        sim.cc_data.fill_BC_all()
        filled = planes(sim.cc_data)
        sim.method_compute_timestep()
        out[pre + "dt_method"] = sim.dt
        sim.compute_timestep()
        out[pre + "dt"] = sim.dt
        rec = captured_evolve(sim)
        new = planes(sim.cc_data)
        assert np.array_equal(new[:4], filled[:4]) and np.all(np.isfinite(new))
        out[pre + "new"] = new[4]
        for kk, v in rec.items():
            out[pre + kk] = v
        g = sim.cc_data.grid
        out[pre + "meta"] = np.array([nx, ny, g.ng, lim, g.dx, g.dy, sim.rp.get_param("driver.cfl")])
        out[pre + "bc"] = np.array([[getattr(sim.cc_data.BCs[n], s) for s in ("xlb", "xrb", "ylb", "yrb")]
                                    for n in NAMES])
        u, v = filled[0], filled[1]
        print(pre, nx, ny, "lim", lim, "dt", sim.dt, "zeros u/v", int((u == 0).sum()), int((v == 0).sum()),
              "signs", int((u > 0).sum()), int((u < 0).sum()), int((v > 0).sum()), int((v < 0).sum()))
    save("advnu_stages", **out)


def slotted_run(nx, ny, nsteps, extra=None):
    p = Pyro("advection_nonuniform")
    p.initialize_problem("slotted", inputs_dict=dict({"mesh.nx": nx, "mesh.ny": ny, "driver.max_steps": nsteps},
                                                     **(extra or {})))
    p.run_sim()
    return p


def gen_runs():
    out = {}
    for k, (nx, ny) in enumerate(((33, 36), (16, 19))):
        for nsteps in (5, 20):
            p = slotted_run(nx, ny, nsteps)
            out[f"r{k}_state{nsteps}"] = planes(p.sim.cc_data)
            out[f"r{k}_t{nsteps}"] = p.sim.cc_data.t
            v = planes(p.sim.cc_data)[1]
            print(f"r{k}", nx, ny, nsteps, "t", p.sim.cc_data.t, "cells with v == 0:", int((v[4:-4, 4:-4] == 0).sum()))
    p = slotted_run(33, 36, 5, {"particles.do_particles": 1, "particles.n_particles": 25})
    out["part_pos5"] = p.sim.particles.get_positions()
    out["part_init"] = p.sim.particles.get_init_positions()
    out["part_state5"] = planes(p.sim.cc_data)
    save("advnu_runs", **out)


def gen_regress():
    """pyro/test.py: advection_nonuniform slotted with inputs.slotted, to completion, and its
    twin with 1e-15 relative noise on the velocities"""
    p = Pyro("advection_nonuniform")
    p.initialize_problem("slotted")
    p.run_sim()
    q = Pyro("advection_nonuniform")
    q.add_problem("generated", prob_noisy(1.e-15), problem_params=dict(slotted.PROBLEM_PARAMS))
    q.initialize_problem("generated", inputs_file=os.path.join(REF, "advection_nonuniform", "problems",
                                                               "inputs.slotted"))
    q.run_sim()
    I = (slice(4, -4), slice(4, -4))
    a, b = planes(q.sim.cc_data)[4][I], planes(p.sim.cc_data)[4][I]
    dev = max_rel_err(a, b)
    print("regress", p.sim.n, p.sim.cc_data.t, "twin", q.sim.n, q.sim.cc_data.t, "twin_dev", dev)
    np.savez_compressed(os.path.join(OUT, "advnu_regress.npz"), n=p.sim.n, t=p.sim.cc_data.t,
                        twin_n=q.sim.n, twin_dev=dev, density=b)
    print("wrote advnu_regress.npz")


def gen_h5():
    src = os.path.join(REF, "advection_nonuniform", "tests", "slotted_0248.h5")
    dst = os.path.join(OUT, "slotted_0248.h5.gz")
    with open(src, "rb") as f, gzip.GzipFile(dst, "wb", compresslevel=9, mtime=0) as z:
        z.write(f.read())
    print("wrote", dst, os.path.getsize(dst) // 1024, "KiB")


if __name__ == "__main__":
    what = sys.argv[1:] or ["stages", "runs", "regress", "h5"]
    os.makedirs(OUT, exist_ok=True)
    for w in what:
        {"stages": gen_stages, "runs": gen_runs, "regress": gen_regress, "h5": gen_h5}[w]()
