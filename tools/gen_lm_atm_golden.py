"""Generate tests/golden/lm_atm_*.npz by RUNNING THE REFERENCE's lm_atm solver (test
infrastructure, build container only):

    cd /tmp && MPLBACKEND=Agg \\
      PYTHONPATH=<repo>/oracle/shim:<reference checkout> \\
      python3 <repo>/tools/gen_lm_atm_golden.py [stages] [runs] [regress] [h5]

The shim of oracle/ replaces numba.njit by the identity.  Nothing of the reference is copied:
its solver is run and its inputs / outputs stored.  Stages are captured by wrapping
LM_atm_interface.mac_vels / rho_states / states and VarCoeffCCMG2d.init_RHS / solve at run time.
  lm_atm_stage<k>.npz one evolve() from a developed state of the off-grid bubble, every stage,
                      for limiter 0 / 1 / 2, proj_type 1 / 2 and two boundary mixes (16^2, 32^2)
  lm_atm_pre.npz      preevolve from the problem's initial conditions and the step after it
  lm_atm_runs.npz     short runs of the off-grid bubble (32^2, 64^2) with their 1e-13 twins
  lm_atm_bubble128.npz  the reference's regression problem (inputs.bubble to t = 1) and its twin
  lm_atm_h5.npz       what the stored lm_bubble_128_0065.h5 holds (needs h5py), and the file
                      itself gzipped as lm_bubble_128_0065.h5.gz (an input of the read test)

The reference imports h5py at import time (util/io_pyro.py); without h5py a stub module stands
in for it and the h5 fixture is skipped.
"""
import gzip
import os
import sys
import tempfile
import types

import numpy as np

try:
    import h5py
except ImportError:
    h5py = None
    sys.modules["h5py"] = types.ModuleType("h5py")

os.chdir(tempfile.mkdtemp())   # Pyro writes inputs.auto into cwd

import pyro.lm_atm.LM_atm_interface as lmi            # noqa: E402
import pyro.lm_atm.simulation as lms                  # noqa: E402
import pyro.multigrid.variable_coeff_MG as vcMG       # noqa: E402
from pyro.pyro_sim import Pyro                        # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
REF = os.path.dirname(os.path.abspath(sys.modules["pyro"].__file__))
NAMES = ["density", "x-velocity", "y-velocity", "eint", "phi-MAC", "phi", "gradp_x", "gradp_y"]
OFFGRID = {"bubble.x_pert": 0.4037, "bubble.y_pert": 0.4519, "bubble.r_pert": 0.0913}
QUIET = {"driver.verbose": 0, "vis.dovis": 0, "io.do_io": 0}

REC = None      # dict the wrappers record into while a step is being captured
SIM = None      # the Simulation being captured


def save(name, **kw):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **kw)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def planes(cc):
    return np.ascontiguousarray(np.moveaxis(np.array(cc.data), -1, 0))


def _wrap(mod, name, fn):
    orig = getattr(mod, name)

    def wrapped(*a, **kw):
        return fn(orig, *a, **kw)
    setattr(mod, name, wrapped)


def _mac_vels(orig, *a):
    out = orig(*a)
    if REC is not None:
        aux = SIM.aux_data
        REC["coeff"] = np.array(aux.get_var("coeff"))
        REC["source"] = np.array(aux.get_var("source_y"))
        REC["umac0"], REC["vmac0"] = np.array(out[0]), np.array(out[1])
    return out


def _rho_states(orig, *a):
    out = orig(*a)
    if REC is not None:
        REC["umac1"], REC["vmac1"] = np.array(a[5]), np.array(a[6])
        REC["rho_xint"], REC["rho_yint"] = np.array(out[0]), np.array(out[1])
    return out


def _states(orig, *a):
    out = orig(*a)
    if REC is not None:
        cc = SIM.cc_data
        REC["rho_new"] = np.array(cc.get_var("density"))
        REC["eint_new"] = np.array(cc.get_var("eint"))
        REC["coeff2"] = np.array(SIM.aux_data.get_var("coeff"))
        for k, n in enumerate(("u_xint", "v_xint", "u_yint", "v_yint")):
            REC[n] = np.array(out[k])
    return out


def _init_rhs(orig, self, data):
    if REC is not None:
        k = REC["nsolve"]
        REC[f"rhs{k}"] = np.array(data)
        if k == REC.get("proj_index", 1):      # the projection: U is the provisional velocity
            cc = SIM.cc_data
            REC["u_prov"] = np.array(cc.get_var("x-velocity"))
            REC["v_prov"] = np.array(cc.get_var("y-velocity"))
    return orig(self, data)


def _solve(orig, self, rtol=1.e-11):
    out = orig(self, rtol=rtol)
    if REC is not None:
        k = REC["nsolve"]
        REC[f"sol{k}"] = np.array(self.get_solution())
        REC[f"eta{k}"] = np.array(self.grids[self.nlevels - 1].get_var("coeffs"))
        REC[f"ncyc{k}"] = self.num_cycles
        REC["nsolve"] = k + 1
    return out


_wrap(lmi, "mac_vels", _mac_vels)
_wrap(lmi, "rho_states", _rho_states)
_wrap(lmi, "states", _states)
_wrap(vcMG.VarCoeffCCMG2d, "init_RHS", _init_rhs)
_wrap(vcMG.VarCoeffCCMG2d, "solve", _solve)


def _perturb(cc, noise, seed=7):
    rng = np.random.default_rng(seed)
    d = cc.get_var("density")
    d.v()[:, :] *= 1.0 + noise * (2.0 * rng.random(d.v().shape) - 1.0)


def make(nx, extra, noise=0.0, noise_pre=0.0, capture_pre=None):
    """Pyro("lm_atm") on the bubble.  noise: relative perturbation of the density of the state
    the time stepping starts from (after preevolve); noise_pre: of the problem's initial
    conditions, before preevolve -- which starts from a velocity that is exactly zero, a state
    made of upwinding ties, and answers 1e-13 with O(1e-2) in grad p (DESIGN); capture_pre:
    dict that receives the stages of preevolve"""
    global REC, SIM
    p = Pyro("lm_atm")
    pre = lms.Simulation.preevolve

    def preevolve(self):
        global REC, SIM
        if noise_pre:
            _perturb(self.cc_data, noise_pre)
        if capture_pre is not None:
            capture_pre["ic"] = planes(self.cc_data)
            REC, SIM = capture_pre, self
            REC["nsolve"] = 0
            REC["proj_index"] = 2
        try:
            pre(self)
        finally:
            REC = SIM = None
    lms.Simulation.preevolve = preevolve
    try:
        p.initialize_problem("bubble", inputs_dict=dict(QUIET, **{"mesh.nx": nx, "mesh.ny": nx}, **extra))
    finally:
        lms.Simulation.preevolve = pre
    if noise:
        _perturb(p.sim.cc_data, noise)
    return p


def base_arrays(sim):
    return {k: np.array(sim.base[n].d) for k, n in (("rho0", "rho0"), ("p0", "p0"), ("beta0", "beta0"),
                                                    ("beta0e", "beta0-edges"))}


def bc_names(sim):
    return np.array([[getattr(sim.cc_data.BCs[n], s) for s in ("xlb", "xrb", "ylb", "yrb")]
                     for n in NAMES])


def meta_of(sim):
    g, rp = sim.cc_data.grid, sim.rp
    return np.array([g.nx, g.ng, rp.get_param("lm-atmosphere.limiter"),
                     rp.get_param("lm-atmosphere.proj_type"), g.dx, g.dy,
                     rp.get_param("lm-atmosphere.grav"), rp.get_param("eos.gamma"),
                     rp.get_param("driver.cfl")])


def stage_case(out, pre, nx, extra, warm):
    """`warm` steps, then one captured single_step"""
    global REC, SIM
    p = make(nx, dict(OFFGRID, **extra))
    for _ in range(warm):
        p.single_step()
    sim = p.sim
    sim.cc_data.fill_BC_all()
    out[pre + "U0"] = planes(sim.cc_data)
    sim.method_compute_timestep()
    out[pre + "dt_method"] = sim.dt
    sim.compute_timestep()
    out[pre + "dt"] = sim.dt
    REC, SIM = {"nsolve": 0, "proj_index": 1}, sim
    try:
        sim.evolve()
        rec = REC
    finally:
        REC = SIM = None
    out[pre + "U1"] = planes(sim.cc_data)
    out[pre + "meta"] = meta_of(sim)
    out[pre + "bc"] = bc_names(sim)
    out[pre + "mesh_bc"] = np.array([sim.rp.get_param("mesh." + k) for k in
                                     ("xlboundary", "xrboundary", "ylboundary", "yrboundary")])
    for k, v in base_arrays(sim).items():
        out[pre + k] = v
    for k, v in rec.items():
        out[pre + k] = v
    print(pre, "ncyc", rec["ncyc0"], rec["ncyc1"], "dt", sim.dt)


def gen_stages():
    out = {}
    walls = {"mesh.xlboundary": "reflect", "mesh.xrboundary": "reflect",
             "mesh.ylboundary": "reflect", "mesh.yrboundary": "outflow"}
    cases = [(16, {"lm-atmosphere.limiter": 2, "lm-atmosphere.proj_type": 2}),
             (16, {"lm-atmosphere.limiter": 1, "lm-atmosphere.proj_type": 1}),
             (16, {"lm-atmosphere.limiter": 0, "lm-atmosphere.proj_type": 2}),
             (16, dict(walls, **{"lm-atmosphere.limiter": 2, "lm-atmosphere.proj_type": 1})),
             (32, {"lm-atmosphere.limiter": 2, "lm-atmosphere.proj_type": 2}),
             (32, dict(walls, **{"lm-atmosphere.limiter": 2, "lm-atmosphere.proj_type": 2}))]
    for k, (nx, extra) in enumerate(cases):      # (one file per case: the size limit of the tree)
        case = {}
        stage_case(case, "", nx, extra, warm=3)
        save(f"lm_atm_stage{k}", **case)
    # preevolve from the problem's initial conditions, with a 1e-13 twin
    for k, nx in enumerate((16, 32)):
        rec = {}
        p = make(nx, dict(OFFGRID), capture_pre=rec)
        pre = f"p{k}_"
        out[pre + "after"] = planes(p.sim.cc_data)
        out[pre + "meta"] = meta_of(p.sim)
        out[pre + "ncyc"] = np.array([rec["ncyc0"], rec["ncyc1"], rec["ncyc2"]])
        out[pre + "ic"] = rec["ic"]
        out[pre + "rhs0"], out[pre + "sol0"] = rec["rhs0"], rec["sol0"]
        for kk, v in base_arrays(p.sim).items():
            out[pre + kk] = v
        q = make(nx, dict(OFFGRID), noise_pre=1.e-13)
        out[pre + "twin"] = np.abs(planes(q.sim.cc_data) - out[pre + "after"]).reshape(8, -1).max(axis=1)
        # ... and one step after it
        q = make(nx, dict(OFFGRID), noise=1.e-13)
        p.single_step()
        q.single_step()
        out[pre + "step1"] = planes(p.sim.cc_data)
        out[pre + "step1_dt"] = p.sim.dt
        out[pre + "step1_twin"] = np.abs(planes(q.sim.cc_data) - out[pre + "step1"]).reshape(8, -1).max(axis=1)
        print(pre, out[pre + "ncyc"], out[pre + "twin"], out[pre + "step1_twin"])
    save("lm_atm_pre", **out)


def run_pair(nx, extra, nsteps, keep):
    """a run and its 1e-13 twin: dts, the states at the steps in `keep`, the per-variable
    maximum difference of the twin at every step"""
    p = make(nx, dict(extra, **{"driver.max_steps": nsteps}))
    q = make(nx, dict(extra, **{"driver.max_steps": nsteps}), noise=1.e-13)
    res = {"after_pre": planes(p.sim.cc_data), "meta": meta_of(p.sim)}
    dts, twin, cyc = [], [], []
    n = 0
    while not p.sim.finished():
        p.single_step()
        q.single_step()
        n += 1
        dts.append(p.sim.dt)
        twin.append(np.abs(planes(q.sim.cc_data) - planes(p.sim.cc_data)).reshape(8, -1).max(axis=1))
        if n in keep:
            res[f"state{n}"] = planes(p.sim.cc_data)
        if n % 10 == 0:
            print("  step", n, "t", p.sim.cc_data.t, flush=True)
    res["dts"] = np.array(dts)
    res["twin"] = np.array(twin)
    res["t"] = p.sim.cc_data.t
    res["nsteps"] = p.sim.n
    return p, q, res


def gen_runs():
    out = {}
    for k, (nx, nsteps, keep) in enumerate(((32, 12, (1, 2, 12)), (64, 12, (12,)))):
        _, _, res = run_pair(nx, OFFGRID, nsteps, keep)
        for kk, v in res.items():
            out[f"r{k}_{kk}"] = v
        print(f"r{k}", nx, "twin at end", res["twin"][-1])
    save("lm_atm_runs", **out)


def gen_regress():
    """pyro/test.py: lm_atm bubble with inputs.bubble, to completion"""
    p, q, res = run_pair(128, {}, 2000, ())
    I = (slice(None), slice(4, -4), slice(4, -4))
    sel = [0, 1, 2, 6, 7]
    gold = planes(p.sim.cc_data)[I][sel]
    twin_end = np.abs(planes(q.sim.cc_data)[I][sel] - gold).reshape(5, -1).max(axis=1)
    save("lm_atm_bubble128", gold=gold, vars=np.array([NAMES[n] for n in sel]), dts=res["dts"],
         nsteps=res["nsteps"], t=res["t"], twin=res["twin"], twin_end=twin_end)
    print("regress", res["nsteps"], res["t"], twin_end)


def gen_h5():
    src = os.path.join(REF, "lm_atm", "tests", "lm_bubble_128_0065.h5")
    dst = os.path.join(OUT, "lm_bubble_128_0065.h5.gz")
    with open(src, "rb") as f, gzip.GzipFile(dst, "wb", compresslevel=9, mtime=0) as z:
        z.write(f.read())
    print("wrote", dst, os.path.getsize(dst) // 1024, "KiB")
    if h5py is None:
        print("h5py is not installed: lm_atm_h5.npz (the file's contents as arrays) skipped")
        return
    with h5py.File(src, "r") as f:
        out = {"t": f.attrs["time"], "nsteps": f.attrs["nsteps"]}
        for n in NAMES:
            out["state_" + n] = f["state"][n]["data"][:, :]
        for n in f["base state"]:
            out["base_" + n] = f["base state"][n][...]
    save("lm_atm_h5", **out)


if __name__ == "__main__":
    what = sys.argv[1:] or ["stages", "runs", "regress", "h5"]
    os.makedirs(OUT, exist_ok=True)
    for w in what:
        {"stages": gen_stages, "runs": gen_runs, "regress": gen_regress, "h5": gen_h5}[w]()
