"""Generate tests/golden/advweno_*.npz by RUNNING THE REFERENCE's advection_weno solver (test
infrastructure, build container only):

    cd /tmp && MPLBACKEND=Agg \\
      PYTHONPATH=<repo>/oracle/shim:<reference checkout> \\
      python3 <repo>/tools/gen_advweno_golden.py [stages] [runs] [regress]

The shim of oracle/ replaces numba.njit by the identity.  Nothing of the reference is copied: its
solver is run and its inputs / outputs stored.  The intermediates of a stage are read from the
frames of the reference's functions when they return, by a profile hook set around evolve(): the
stage start after its fill and F_x, F_y (locals of fluxes()), the reconstructed positive part of
the split flux of every pencil (flux_p_r, a local of fvs(): assembled into one plane per
direction), k_s (the return value of substep()).
  advweno_stages.npz   one evolve() per case: the density before the fill (ghost cells hold junk),
                       per stage the stage start after its fill, flux_p_r in x and y, F_x, F_y and
                       k_s, the density after the step with its ghost frame, the dt of the step and
                       that of method_compute_timestep (they differ at zero velocity, where the
                       driver cuts the step to tmax), alpha as fluxes() forms it; `twin_dev`: what
                       the step of the reference differs by when the input carries 1e-15 relative
                       noise
  advweno_runs.npz     5 and 20 steps of `smooth` through Pyro(...).run_sim() for both orders, and
                       5 steps with 25 tracer particles
  advweno_regress.npz  `smooth` with the advection solver's inputs.smooth (32 x 32, to t = 1) for
                       both orders: step count, time, density, and the twins with 1e-15 relative
                       noise on the initial data: `twin_dev`, the yardstick of the contracted build
                       (the reference stores no output file for this solver)

How the reference rounds.  The kernel of csrc/advection_rk.hip repeats weno_upwind under three
assumptions, and this generator verifies them BEFORE it writes advweno_stages.npz, on every call
of weno_upwind of the recorded steps, with exact rational arithmetic (fractions.Fraction; a
Fraction converts to the nearest double):
  np.dot(w, q_stencils)   is the chain fma(w_k, s_k, acc) from acc = 0, k ascending
  np.sum(alpha)           is the sum from left to right
  beta_k**2               is the C library's pow(beta_k, 2.0) (math.pow) -- NOT always the product
                          beta_k * beta_k: pow() is not correctly rounded, and in about one call
                          of a thousand the two differ by a unit in the last place.  The kernel
                          repeats that pow() operation for operation (csrc/libm_pow2.h); the
                          generator counts the calls in which it is not the product and wants
                          some among the recorded cases, so that the tests hold the kernel to it
If one of them fails the generator stops and says which: the kernel has to change then, not the
tests.

This checkout of the reference has no problems directory under advection_weno: the problems are
the advection solver's, registered by add_problem(), with that solver's inputs.smooth.

The reference imports h5py at import time (util/io_pyro.py); without h5py a stub module stands
in for it.
"""
import math
import os
import sys
import tempfile
import types
from fractions import Fraction

import numpy as np

try:
    import h5py  # noqa: F401
except ImportError:
    sys.modules["h5py"] = types.ModuleType("h5py")

os.chdir(tempfile.mkdtemp())   # Pyro writes inputs.auto into cwd

import pyro.advection_weno.fluxes as flx                      # noqa: E402
from pyro.advection.problems import smooth, tophat            # noqa: E402
from pyro.mesh import reconstruction                          # noqa: E402
from pyro.pyro_sim import Pyro                                # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
REF = os.path.dirname(os.path.abspath(sys.modules["pyro"].__file__))
INPUTS_SMOOTH = os.path.join(REF, "advection", "problems", "inputs.smooth")
POLICY = {"driver.init_tstep_factor": 1.0, "driver.max_dt_change": 1.e33, "driver.tmax": 1.e3}
SIDES = ("mesh.xlboundary", "mesh.xrboundary", "mesh.ylboundary", "mesh.yrboundary")
PERIODIC = dict.fromkeys(SIDES, "periodic")
OUTFLOW = dict.fromkeys(SIDES, "outflow")
WALLS_X = dict(zip(SIDES, ("reflect", "reflect", "outflow", "outflow")))
WALLS_Y = dict(zip(SIDES, ("outflow", "outflow", "reflect", "reflect")))
NG = 4
PLANES = ("start", "fpr_x", "fpr_y", "F_x", "F_y", "k")


def save(name, **kw):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **kw)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def max_rel_err(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def dens(cc):
    return np.array(cc.get_var("density"))


class constant:
    """exactly one value everywhere: every smoothness indicator is 0"""
    @staticmethod
    def init_data(my_data, rp):
        my_data.get_var("density")[:, :] = 1.0


def problem(base, amp, seed, noise=0.0):
    """the problem's field plus random structure of amplitude amp everywhere, junk in the ghost
    cells, optional relative noise"""
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


def make(init, extra, inputs_file=None, name="generated"):
    p = Pyro("advection_weno")
    p.add_problem(name, init, problem_params={})
    p.initialize_problem(name, inputs_file=inputs_file, inputs_dict=extra)
    return p


# ---- how the reference rounds ------------------------------------------------------------------

class Rounding:
    """the three assumptions, checked on a returning frame of weno_upwind"""
    WHAT = {"dot": "np.dot(w, q_stencils) is not the chain of fused multiply-adds from 0",
            "sum": "np.sum(alpha) is not the sum from left to right",
            "pow": "beta**2 is not the C library's pow(beta, 2.0)"}

    def __init__(self):
        self.calls = 0
        self.not_product = 0      # calls in which some beta**2 is not the correctly rounded square
        self.bad = dict.fromkeys(self.WHAT, 0)

    def check(self, loc, result):
        self.calls += 1
        C = reconstruction.C_all[loc["order"]]
        alpha, beta, s, w = loc["alpha"], loc["beta"], loc["q_stencils"], loc["w"]
        sq = [math.pow(float(b), 2.0) for b in beta]
        if any(float(alpha[k]) != float(C[k]) / (1e-16 + sq[k]) for k in range(len(C))):
            self.bad["pow"] += 1
        self.not_product += any(sq[k] != float(Fraction(float(beta[k])) ** 2) for k in range(len(C)))
        tot = float(alpha[0])
        for k in range(1, len(C)):
            tot = float(Fraction(tot) + Fraction(float(alpha[k])))
        if not np.array_equal(alpha / tot, w):
            self.bad["sum"] += 1
        acc = 0.0
        for k in range(len(C)):
            acc = float(Fraction(float(w[k])) * Fraction(float(s[k])) + Fraction(acc))
        if acc != float(result):
            self.bad["dot"] += 1

    def verdict(self):
        print("rounding of weno_upwind:", self.calls, "calls,", self.bad, "; beta**2 is not the product in",
              self.not_product)
        for key, n in self.bad.items():
            if n:
                sys.exit(f"ROUNDING ASSUMPTION FAILED: {self.WHAT[key]} in {n} of {self.calls} calls of "
                         "weno_upwind: the kernel has to change (csrc/advection_rk.hip), nothing is written")
        assert self.calls > 0 and self.not_product > 0


def captured_evolve(sim, rounding=None):
    """evolve() with the intermediates of every stage"""
    stages, pencils = [], []
    vcode, fcode, scode = flx.fvs.__code__, flx.fluxes.__code__, type(sim).substep.__code__
    wcode = reconstruction.weno_upwind.__code__

    def hook(frame, event, arg):
        if event != "return":
            return
        code = frame.f_code
        if code is wcode:
            if rounding is not None:
                rounding.check(frame.f_locals, arg)
        elif code is vcode:
            pencils.append(np.array(frame.f_locals["flux_p_r"]))
        elif code is fcode:
            loc = frame.f_locals
            g = loc["myg"]
            assert len(pencils) == g.qy + g.qx     # x pencils (one per column), then y pencils
            stages.append({"start": dens(loc["my_data"]),
                           "fpr_x": np.stack(pencils[:g.qy], axis=1), "fpr_y": np.stack(pencils[g.qy:], axis=0),
                           "F_x": np.array(loc["F_x"]), "F_y": np.array(loc["F_y"]),
                           "alpha": float(loc["alpha"])})
            pencils.clear()
        elif code is scode:
            stages[-1]["k"] = np.array(arg)
    sys.setprofile(hook)
    try:
        sim.evolve()
    finally:
        sys.setprofile(None)
    return stages


# (nx, ny, weno_order, method, (u, v), sides, base problem, amplitude of the random structure)
CASES = [
    (33, 36, 3, "RK4", (1.0, 1.0), PERIODIC, smooth, 1.0),
    (16, 19, 2, "TVD2", (-1.0, 0.5), OUTFLOW, tophat, 0.3),
    (16, 19, 3, "TVD3", (0.7, -1.0), WALLS_X, tophat, 0.0),
    (19, 16, 2, "RK4", (-1.0, 0.0), WALLS_Y, smooth, 1.0),
    (8, 8, 3, "TVD2", (0.0, 1.0), WALLS_X, smooth, 1.0),
    (8, 8, 2, "TVD3", (0.0, 0.0), OUTFLOW, smooth, 1.0),
    (4, 5, 3, "RK2", (1.0, 1.0), PERIODIC, smooth, 1.0),
    (4, 5, 2, "RK4", (-1.0, 0.5), PERIODIC, tophat, 1.0),
    (8, 8, 3, "RK4", (1.0, 1.0), PERIODIC, constant, 0.0),
    (8, 8, 2, "RK2", (0.7, -1.0), OUTFLOW, constant, 0.0),
    (16, 19, 3, "RK2", (1.0, 1.0), PERIODIC, constant, 1.e-4),
    (8, 8, 2, "TVD2", (-1.0, 0.5), OUTFLOW, constant, 1.e-4),
    (8, 8, 3, "RK4", (0.0, 0.0), PERIODIC, tophat, 1.0),
    (16, 19, 3, "TVD2", (-1.0, 0.5), OUTFLOW, tophat, 0.0),
]


def one_step(case, seed, noise=0.0, rounding=None):
    nx, ny, order, method, (u, v), sides, base, amp = case
    p = make(problem(base, amp, seed, noise),
             dict(POLICY, **sides, **{"mesh.nx": nx, "mesh.ny": ny, "advection.weno_order": order,
                                      "advection.u": u, "advection.v": v,
                                      "advection.temporal_method": method}))
    sim = p.sim
    before = dens(sim.cc_data)
    sim.method_compute_timestep()
    dt_method = sim.dt
    sim.compute_timestep()
    # (zero velocity: the advective step is SMALL's inverse, the driver cuts it to tmax)
    assert sim.dt == dt_method or ((u, v) == (0.0, 0.0) and sim.dt == POLICY["driver.tmax"])
    sim.dt_method = dt_method
    stages = captured_evolve(sim, rounding)
    return sim, before, stages, dens(sim.cc_data)


def gen_stages():
    out = {"ncases": len(CASES)}
    rounding = Rounding()
    I = (slice(NG, -NG), slice(NG, -NG))
    for k, case in enumerate(CASES):
        nx, ny, order, method, (u, v), sides, base, amp = case
        sim, before, stages, new = one_step(case, 100 + k, rounding=rounding)
        assert np.all(np.isfinite(new)) and not np.array_equal(new, before)
        pre = f"c{k}_"
        out[pre + "Uin"] = before
        out[pre + "new"] = new
        out[pre + "dt"] = sim.dt
        out[pre + "dt_method"] = sim.dt_method
        for s, rec in enumerate(stages):
            assert rec["alpha"] == stages[0]["alpha"]
            for key in PLANES:
                out[f"{pre}s{s}_{key}"] = rec[key]
        g = sim.cc_data.grid
        out[pre + "meta"] = np.array([nx, ny, g.ng, order, 5, g.dx, g.dy, u, v,
                                      sim.rp.get_param("driver.cfl"), len(stages), stages[0]["alpha"], amp])
        out[pre + "method"] = np.array(method)
        out[pre + "data"] = np.array(base.__name__.split(".")[-1])
        bc = sim.cc_data.BCs["density"]
        out[pre + "bc"] = np.array([bc.xlb, bc.xrb, bc.ylb, bc.yrb])
        if (u, v) == (0.0, 0.0):
            assert stages[0]["alpha"] == 0.0 and np.array_equal(new[I], before[I])
        # the reference's own sensitivity of this step to 1e-15 relative noise on its input
        _, _, _, twin = one_step(case, 100 + k, noise=1.e-15)
        out[pre + "twin_dev"] = max_rel_err(twin[I], new[I])
        # (structure of 1e-4 on a constant: beta^2 is of the size of the 1e-16 beside it, the
        # weights -- and the reference's own step -- feel noise on the input most there; the
        # tests hold such a case to 10 x its twin_dev where that is above 1e-12)
        small = base is constant and 0.0 < amp <= 1.e-4
        assert out[pre + "twin_dev"] <= (1.e-10 if small else 1.e-12), (k, out[pre + "twin_dev"])
        print(pre, nx, ny, "order", order, method, (u, v), base.__name__, amp, "dt", sim.dt, "stages", len(stages),
              "twin_dev %.2e" % out[pre + "twin_dev"])
    rounding.verdict()
    save("advweno_stages", **out)


def smooth_run(order, nx, ny, nsteps, extra=None):
    p = make(smooth.init_data, dict({"mesh.nx": nx, "mesh.ny": ny, "driver.max_steps": nsteps,
                                     "advection.weno_order": order}, **(extra or {})),
             inputs_file=INPUTS_SMOOTH, name="smooth")
    p.run_sim()
    return p


def gen_runs():
    out = {}
    for order in (2, 3):
        for k, (nx, ny), steps in ((0, (33, 36), (5,)), (1, (16, 19), (5, 20))):
            for nsteps in steps:
                p = smooth_run(order, nx, ny, nsteps)
                assert p.sim.n == nsteps
                out[f"o{order}_r{k}_state{nsteps}"] = dens(p.sim.cc_data)
                out[f"o{order}_r{k}_t{nsteps}"] = p.sim.cc_data.t
                print(f"o{order}_r{k}", nx, ny, nsteps, "t", p.sim.cc_data.t)
        p = smooth_run(order, 33, 36, 5, {"particles.do_particles": 1, "particles.n_particles": 25})
        # (the data do not feel the particles)
        assert np.array_equal(dens(p.sim.cc_data), out[f"o{order}_r0_state5"])
        out[f"o{order}_part_pos5"] = p.sim.particles.get_positions()
        out[f"o{order}_part_init"] = p.sim.particles.get_init_positions()
    save("advweno_runs", **out)


def noisy_smooth(noise, seed=11):
    def init(my_data, rp):
        smooth.init_data(my_data, rp)
        d = my_data.get_var("density")
        d[:, :] = d * (1.0 + noise * (2.0 * np.random.default_rng(seed).random(d.shape) - 1.0))
    return init


def gen_regress():
    """`smooth` with inputs.smooth to completion for both orders, and the twins with 1e-15
    relative noise on the initial data"""
    out = {}
    I = (slice(NG, -NG), slice(NG, -NG))
    for order in (2, 3):
        extra = {"advection.weno_order": order}
        p = make(smooth.init_data, extra, inputs_file=INPUTS_SMOOTH, name="smooth")
        p.run_sim()
        q = make(noisy_smooth(1.e-15), extra, inputs_file=INPUTS_SMOOTH)
        q.run_sim()
        a, b = dens(q.sim.cc_data)[I], dens(p.sim.cc_data)[I]
        dev = max_rel_err(a, b)
        print("advection_weno order", order, "regress", p.sim.n, p.sim.cc_data.t, "twin", q.sim.n, "twin_dev", dev)
        pre = f"o{order}_"
        # (n, t, the twin's n, twin_dev in one array: every entry of the archive costs its header)
        out.update({pre + "meta": np.array([p.sim.n, p.sim.cc_data.t, q.sim.n, dev]), pre + "density": b})
    save("advweno_regress", **out)


if __name__ == "__main__":
    what = sys.argv[1:] or ["stages", "runs", "regress"]
    os.makedirs(OUT, exist_ok=True)
    for w in what:
        {"stages": gen_stages, "runs": gen_runs, "regress": gen_regress}[w]()
