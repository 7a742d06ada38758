"""Generate tests/golden/advrk_*.npz and the two stored regression files by RUNNING THE REFERENCE's
advection_rk and advection_fv4 solvers (test infrastructure, build container only):

    cd /tmp && MPLBACKEND=Agg \\
      PYTHONPATH=<repo>/oracle/shim:<reference checkout> \\
      python3 <repo>/tools/gen_advrk_golden.py [stages] [runs] [regress] [h5]

The shim of oracle/ replaces numba.njit by the identity.  Nothing of the reference is copied: its
solvers are run and their inputs / outputs stored.  The intermediates of a stage (the stage start
after its fill, the face values and fluxes -- locals of fluxes() --, k_s -- the return value of
substep()) are read from the frames of those functions when they return, by a profile hook set
around evolve().
  advrk_stages.npz   one evolve() per case: the density before the fill (ghost cells hold junk:
                     the step under test has to apply the boundary rules), per stage the stage
                     start after its fill, a_x, a_y, F_x, F_y and k_s, the density after the step
                     with its ghost frame, dt of method_compute_timestep; `twin_dev`: what the
                     step of the reference differs by when the input carries 1e-15 relative noise
  advrk_runs.npz     5 and 20 steps of `smooth` through Pyro(...).run_sim() at 33 x 36 and
                     16 x 19 for both solvers (advection_fv4: preevolve included), and 5 steps
                     with tracer particles
  advrk_regress.npz  the two regression runs (inputs.smooth to the end: step count, time,
                     density) and their twins with 1e-15 relative noise on the initial data:
                     `twin_dev`, the yardstick of the contracted build
  advrk_smooth_0081.h5, advfv4_smooth_0081.h5   the reference's stored regression files

Which branch of fourth_order.states a cell takes is decided again here (limiter_branch, written
for this purpose from McCorquodale & Colella's Eqs. 24-32 as the reference applies them), and the
generator asserts that every branch is taken by some recorded case.

The reference imports h5py at import time (util/io_pyro.py); without h5py a stub module stands
in for it.
"""
import os
import shutil
import sys
import tempfile
import types

import numpy as np

try:
    import h5py  # noqa: F401
except ImportError:
    sys.modules["h5py"] = types.ModuleType("h5py")

os.chdir(tempfile.mkdtemp())   # Pyro writes inputs.auto into cwd

import pyro.advection_fv4.fluxes as flx4                      # noqa: E402
import pyro.advection_rk.fluxes as flx2                       # noqa: E402
from pyro.advection.problems import smooth, tophat            # noqa: E402
from pyro.pyro_sim import Pyro                                # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
REF = os.path.dirname(os.path.abspath(sys.modules["pyro"].__file__))
SOLVER = {2: "advection_rk", 4: "advection_fv4"}
POLICY = {"driver.init_tstep_factor": 1.0, "driver.max_dt_change": 1.e33, "driver.tmax": 1.e3}
SIDES = ("mesh.xlboundary", "mesh.xrboundary", "mesh.ylboundary", "mesh.yrboundary")
PERIODIC = dict.fromkeys(SIDES, "periodic")
OUTFLOW = dict.fromkeys(SIDES, "outflow")
WALLS_X = dict(zip(SIDES, ("reflect", "reflect", "outflow", "outflow")))
WALLS_Y = dict(zip(SIDES, ("outflow", "outflow", "reflect", "reflect")))
NG = 4


def save(name, **kw):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **kw)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def max_rel_err(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def dens(cc):
    return np.array(cc.get_var("density"))


def problem(base, amp, seed, noise=0.0):
    """the problem's field plus random structure of amplitude amp everywhere (the cells next to
    the ghost frame matter to the update), junk in the ghost cells, optional relative noise"""
    def init(my_data, rp):
        base.init_data(my_data, rp)
        rng = np.random.default_rng(seed)
        d = my_data.get_var("density")
        d[:, :] = d + amp * rng.random(d.shape)
        junk = 3.0 * rng.random(d.shape) - 1.0
        inner = np.zeros(d.shape, dtype=bool)
        inner[NG:-NG, NG:-NG] = True
        d[:, :] = np.where(inner, d, junk)
        if noise:
            d[:, :] = d * (1.0 + noise * (2.0 * np.random.default_rng(seed + 1000).random(d.shape) - 1.0))
    return init


class cubic:
    """a cubic profile in cell units along both directions, extrema two cells from the
    inflection points: the limiter finds an extremum whose third differences do not vary
    (the one branch of fourth_order.states that random and top-hat data never take)"""
    @staticmethod
    def init_data(my_data, rp):
        g = my_data.grid
        xi = np.arange(g.qx, dtype=np.float64)[:, None] - (NG + g.nx // 2 - 2)
        eta = np.arange(g.qy, dtype=np.float64)[None, :] - (NG + g.ny // 2 - 2)
        d = my_data.get_var("density")
        d[:, :] = (xi**3 - 12.0 * xi) + (eta**3 - 12.0 * eta)


def make(scheme, init, extra):
    p = Pyro(SOLVER[scheme])
    p.add_problem("generated", init, problem_params={})
    p.initialize_problem("generated", inputs_dict=extra)
    return p


def captured_evolve(sim, scheme):
    """evolve() with the intermediates of every stage"""
    stages = []
    fcode = (flx2 if scheme == 2 else flx4).fluxes.__code__
    scode = type(sim).substep.__code__

    def hook(frame, event, arg):
        if event != "return":
            return
        if frame.f_code is fcode:
            loc = frame.f_locals
            stages.append({"start": dens(loc["my_data"]),
                           **{k: np.array(loc[k]) for k in ("a_x", "a_y", "F_x", "F_y")}})
        elif frame.f_code is scode:
            stages[-1]["k"] = np.array(arg)
    sys.setprofile(hook)
    try:
        sim.evolve()
    finally:
        sys.setprofile(None)
    return stages


# ---- which branch of fourth_order.states a cell takes -----------------------------------------

BRANCHES = ("smooth_none", "smooth_ar", "smooth_al", "ext_keep_rho", "ext_keep_d3a", "ext_both",
            "ext_ar", "ext_al", "ext_neither", "lim_zero", "lim_nonzero", "rho_zero")


def limiter_branch(w, top_zero):
    """the decisions of the limiter for the cell in the middle of w = a[c-3 .. c+3]"""
    taken = set()
    f = lambda m: 7. / 12. * (w[m - 1] + w[m]) - 1. / 12. * (w[m - 2] + w[m + 1])     # noqa: E731
    lo, hi, a = f(3), f(4), w[3]
    dm, dp = a - lo, hi - a
    curv_f = 6.0 * (lo - 2.0 * a + hi)
    curv = [w[m - 1] - 2.0 * w[m] + w[m + 1] for m in range(1, 6)]       # cells c-2 .. c+2
    if dm * dp <= 0.0 or (a - w[1]) * (w[5] - a) <= 0.0:
        s = np.copysign(1.0, curv[2])
        if all(np.copysign(1.0, x) == s for x in (curv[1], curv[3], curv_f)):
            lim = s * min(abs(curv_f), 1.25 * abs(curv[1]), 1.25 * abs(curv[2]), 1.25 * abs(curv[3]))
            taken.add("lim_nonzero")
        else:
            lim = 0.0
            taken.add("lim_zero")
        if abs(curv_f) <= 1.e-12 * max(abs(x) for x in w[1:6]):
            rho = 0.0
            taken.add("rho_zero")
        else:
            rho = lim / curv_f
        if not rho < 1.0 - 1.e-12:
            taken.add("ext_keep_rho")
            return taken
        third = [curv[1] - curv[0], curv[2] - curv[1], curv[3] - curv[2],
                 0.0 if top_zero else curv[4] - curv[3]]
        if not 0.1 * max(abs(min(third)), abs(max(third))) <= max(third) - min(third):
            taken.add("ext_keep_d3a")
        elif dm * dp < 0.0:
            taken.add("ext_both")
        elif abs(dm) >= 2.0 * abs(dp):
            taken.add("ext_ar")
        elif abs(dp) >= 2.0 * abs(dm):
            taken.add("ext_al")
        else:
            taken.add("ext_neither")
    else:
        big_m, big_p = abs(dm) >= 2.0 * abs(dp), abs(dp) >= 2.0 * abs(dm)
        taken.add("smooth_ar" if big_m else ("smooth_al" if big_p else "smooth_none"))
    return taken


def branches_of(a, nx, ny):
    """over the cells whose limited states the update reads, both sweeps"""
    taken = set()
    for i in range(NG - 1, NG + nx + 1):
        for j in range(NG - 1, NG + ny + 1):
            if NG <= j < NG + ny:
                taken |= limiter_branch(a[i - 3:i + 4, j], False)
            if NG <= i < NG + nx:
                taken |= limiter_branch(a[i, j - 3:j + 4], j == NG + ny)
    return taken


# (nx, ny, scheme, limiter, method, (u, v), sides, base problem, amplitude of the random structure)
CASES = [
    (33, 36, 2, 2, "RK4", (1.0, 1.0), PERIODIC, smooth, 1.0),
    (16, 19, 2, 1, "TVD3", (-1.0, 0.5), OUTFLOW, tophat, 1.0),
    (4, 5, 2, 0, "RK2", (0.7, -1.0), PERIODIC, smooth, 1.0),
    (8, 8, 2, 2, "TVD2", (0.0, 1.0), WALLS_X, smooth, 1.0),
    (16, 19, 2, 2, "RK4", (-1.0, 0.0), WALLS_Y, tophat, 1.0),
    (33, 36, 4, 1, "RK4", (1.0, 1.0), PERIODIC, tophat, 1.0),
    (16, 19, 4, 0, "TVD3", (-1.0, 0.5), OUTFLOW, smooth, 1.0),
    (4, 5, 4, 1, "RK2", (0.7, -1.0), PERIODIC, smooth, 1.0),
    (8, 8, 4, 1, "TVD2", (0.0, 1.0), WALLS_X, smooth, 1.0),
    (19, 16, 4, 1, "RK4", (-1.0, 0.0), WALLS_Y, tophat, 0.0),
    (16, 19, 4, 1, "RK4", (1.0, 1.0), PERIODIC, smooth, 0.0),
    (16, 19, 4, 1, "TVD3", (0.7, -1.0), OUTFLOW, tophat, 0.01),
    (16, 19, 4, 0, "RK4", (0.0, -1.0), WALLS_Y, tophat, 1.0),
    (16, 19, 4, 1, "RK4", (1.0, -0.5), OUTFLOW, cubic, 0.0),
]


def one_step(case, seed, noise=0.0):
    nx, ny, scheme, lim, method, (u, v), sides, base, amp = case
    p = make(scheme, problem(base, amp, seed, noise),
             dict(POLICY, **sides, **{"mesh.nx": nx, "mesh.ny": ny, "advection.limiter": lim,
                                      "advection.u": u, "advection.v": v,
                                      "advection.temporal_method": method}))
    sim = p.sim
    before = dens(sim.cc_data)
    sim.method_compute_timestep()
    dt_method = sim.dt
    sim.compute_timestep()
    assert sim.dt == dt_method
    stages = captured_evolve(sim, scheme)
    return sim, before, stages, dens(sim.cc_data)


def gen_stages():
    out = {"ncases": len(CASES)}
    seen = set()
    for k, case in enumerate(CASES):
        nx, ny, scheme, lim, method, (u, v), sides, base, amp = case
        sim, before, stages, new = one_step(case, 100 + k)
        assert np.all(np.isfinite(new)) and not np.array_equal(new, before)
        pre = f"c{k}_"
        out[pre + "Uin"] = before
        out[pre + "new"] = new
        out[pre + "dt"] = sim.dt
        for s, rec in enumerate(stages):
            for key, val in rec.items():
                out[f"{pre}s{s}_{key}"] = val
        g = sim.cc_data.grid
        out[pre + "meta"] = np.array([nx, ny, g.ng, lim, scheme, g.dx, g.dy, u, v,
                                      sim.rp.get_param("driver.cfl"), len(stages)])
        out[pre + "method"] = np.array(method)
        bc = sim.cc_data.BCs["density"]
        out[pre + "bc"] = np.array([bc.xlb, bc.xrb, bc.ylb, bc.yrb])
        # the reference's own sensitivity of this step to 1e-15 relative noise on its input
        _, _, _, twin = one_step(case, 100 + k, noise=1.e-15)
        I = (slice(NG, -NG), slice(NG, -NG))
        out[pre + "twin_dev"] = max_rel_err(twin[I], new[I])
        assert out[pre + "twin_dev"] <= 1.e-12, (k, out[pre + "twin_dev"])
        took = set()
        if scheme == 4 and lim != 0:
            for rec in stages:
                took |= branches_of(rec["start"], nx, ny)
            seen |= took
        print(pre, nx, ny, "scheme", scheme, "lim", lim, method, (u, v), "dt", sim.dt, "stages", len(stages),
              "twin_dev %.2e" % out[pre + "twin_dev"], sorted(took))
    missing = set(BRANCHES) - seen
    assert not missing, f"no recorded case takes {sorted(missing)}"
    save("advrk_stages", **out)


def smooth_run(scheme, nx, ny, nsteps, extra=None):
    p = Pyro(SOLVER[scheme])
    p.initialize_problem("smooth", inputs_dict=dict({"mesh.nx": nx, "mesh.ny": ny, "driver.max_steps": nsteps},
                                                    **(extra or {})))
    p.run_sim()
    return p


def gen_runs():
    out = {}
    for scheme in (2, 4):
        for k, (nx, ny) in enumerate(((33, 36), (16, 19))):
            for nsteps in (5, 20):
                p = smooth_run(scheme, nx, ny, nsteps)
                assert p.sim.n == nsteps
                out[f"s{scheme}_r{k}_state{nsteps}"] = dens(p.sim.cc_data)
                out[f"s{scheme}_r{k}_t{nsteps}"] = p.sim.cc_data.t
                print(f"s{scheme}_r{k}", nx, ny, nsteps, "t", p.sim.cc_data.t)
        p = smooth_run(scheme, 33, 36, 5, {"particles.do_particles": 1, "particles.n_particles": 25})
        out[f"s{scheme}_part_pos5"] = p.sim.particles.get_positions()
        out[f"s{scheme}_part_init"] = p.sim.particles.get_init_positions()
        out[f"s{scheme}_part_state5"] = dens(p.sim.cc_data)
    save("advrk_runs", **out)


def noisy_smooth(noise, seed=11):
    def init(my_data, rp):
        smooth.init_data(my_data, rp)
        d = my_data.get_var("density")
        d[:, :] = d * (1.0 + noise * (2.0 * np.random.default_rng(seed).random(d.shape) - 1.0))
    return init


def gen_regress():
    """pyro/test.py: advection_rk and advection_fv4 smooth with inputs.smooth, to completion, and
    their twins with 1e-15 relative noise on the initial data"""
    out = {}
    I = (slice(NG, -NG), slice(NG, -NG))
    for scheme in (2, 4):
        p = Pyro(SOLVER[scheme])
        p.initialize_problem("smooth")
        p.run_sim()
        q = Pyro(SOLVER[scheme])
        q.add_problem("generated", noisy_smooth(1.e-15), problem_params={})
        q.initialize_problem("generated", inputs_file=os.path.join(REF, SOLVER[scheme], "problems", "inputs.smooth"))
        q.run_sim()
        a, b = dens(q.sim.cc_data)[I], dens(p.sim.cc_data)[I]
        dev = max_rel_err(a, b)
        print(SOLVER[scheme], "regress", p.sim.n, p.sim.cc_data.t, "twin", q.sim.n, "twin_dev", dev)
        pre = f"s{scheme}_"
        out.update({pre + "n": p.sim.n, pre + "t": p.sim.cc_data.t, pre + "twin_n": q.sim.n,
                    pre + "twin_dev": dev, pre + "density": b})
    save("advrk_regress", **out)


def gen_h5():
    for solver, name in (("advection_rk", "advrk_smooth_0081.h5"), ("advection_fv4", "advfv4_smooth_0081.h5")):
        dst = os.path.join(OUT, name)
        shutil.copyfile(os.path.join(REF, solver, "tests", "smooth_0081.h5"), dst)
        print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    what = sys.argv[1:] or ["stages", "runs", "regress", "h5"]
    os.makedirs(OUT, exist_ok=True)
    for w in what:
        {"stages": gen_stages, "runs": gen_runs, "regress": gen_regress, "h5": gen_h5}[w]()
