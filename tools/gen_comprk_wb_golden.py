"""Generate tests/golden/comp_rk_wb.npz by RUNNING THE REFERENCE's compressible_rk solver with
compressible.well_balanced = 1 (test infrastructure, build container only):

    cd /tmp && MPLBACKEND=Agg \\
      PYTHONPATH=<repo>/oracle/shim:<reference checkout> \\
      python3 <repo>/tools/gen_comprk_wb_golden.py

The shim of oracle/ replaces numba.njit by the identity.  Nothing of the reference is copied: its
solver is run and its inputs / outputs stored.  The intermediates of the first stage of the first
step are read by a profile hook set around evolve(): the plane reconstruction.well_balance()
returns (the y slope of the pressure less its hydrostatic part) and, from the frame of substep()
when it returns, the ghost-filled stage start and k.

The problem is registered with add_problem() (the reference's `hse` problem does not initialise
on grids this small): a stratified atmosphere in discrete hydrostatic balance,
    rho = 1 + 0.5 exp(-2 y)                                            on the whole array
    p[:, j] = p[:, j-1] + 0.5 dy (rho[:, j-1] + rho[:, j]) grav        upward from p[:, 0] = 5 + |grav|
then relative random structure of amplitude amp on rho and p and velocities amp (2 r - 1), seeded
per case; the energy from the gamma law.  tests/test_comprk_wellbalanced.py repeats it for the
equilibrium runs and takes the recorded `ic` everywhere else.

Per case c<k>_:
  meta, bc, method, riemann, sponge, drv   as in comp_rk.npz (oracle/gen_golden.py)
  ic                 the initial state with its unfilled ghost frame
  U0, wb, k          first stage of the first step: the ghost-filled stage start, the plane of
                     well_balance(), the k of substep()
  dts, final         the dt of every step, the state after the last
  plain_dev          max over the interior of |final - final of the same run with the option off|
                     / per-variable max (at least 1e-3): what a device path that ignores the option would miss by
  twin_dev           the same against a run whose initial data carry 1e-15 relative noise: the
                     reference's own sensitivity, the yardstick of the contracted build
rest<k>_wb, rest<k>_plain for cases 0 and 3: max |y-momentum| after 20 steps from the atmosphere at
rest (amp 0) with and without the option.

Nothing is written unless every plain_dev > 1e-6, every twin_dev <= 1e-11 and
rest_wb <= 1e-9 rest_plain.

The reference imports h5py at import time (util/io_pyro.py); without h5py a stub module stands in
for it.
"""
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

from pyro.mesh import reconstruction                          # noqa: E402
from pyro.pyro_sim import Pyro                                # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
SIDES = ("mesh.xlboundary", "mesh.xrboundary", "mesh.ylboundary", "mesh.yrboundary")
HSE = dict(zip(SIDES, ("periodic", "periodic", "hse", "hse")))
PERIODIC = dict.fromkeys(SIDES, "periodic")
REFLECT = dict.fromkeys(SIDES, "reflect")
OUTFLOW = dict.fromkeys(SIDES, "outflow")
MIXED = dict(zip(SIDES, ("outflow", "reflect", "hse", "hse")))
SPONGE = {"sponge.do_sponge": 1}      # (the solver's default densities: the sponge is on and adds nothing here)
NSTEPS = 3
NREST = 20

# (nx, ny, sides, Riemann solver, method, amp, extra parameters)
CASES = [
    (8, 24, HSE, "HLLC", "RK4", 0.0, {}),
    (4, 4, PERIODIC, "HLLC", "RK2", 0.2, {}),
    (5, 7, HSE, "HLLC", "TVD3", 0.05, {}),
    (4, 258, HSE, "CGF", "RK2", 0.05, {}),
    (70, 4, REFLECT, "HLLC", "TVD2", 0.2, {}),
    (40, 9, REFLECT, "CGF", "RK4", 0.2, {"compressible.use_flattening": 0}),
    (12, 36, HSE, "HLLC_lm", "TVD2", 0.02, {}),
    (9, 8, OUTFLOW, "HLLC", "RK4", 0.3, {"compressible.grav": 0.0}),
    (6, 10, MIXED, "HLLC", "RK4", 0.1, {"compressible.grav": 2.5}),
    (16, 16, REFLECT, "HLLC", "RK4", 0.3, SPONGE),
]
REST_CASES = (0, 3)


def atmosphere(amp, seed, noise=0.0):
    def init(my_data, rp):
        g = my_data.grid
        gamma, grav = rp.get_param("eos.gamma"), rp.get_param("compressible.grav")
        dens, ener = my_data.get_var("density"), my_data.get_var("energy")
        xmom, ymom = my_data.get_var("x-momentum"), my_data.get_var("y-momentum")
        rho = np.empty((g.qx, g.qy))
        rho[:, :] = (1.0 + 0.5 * np.exp(-2.0 * np.asarray(g.y)))[np.newaxis, :]
        p = np.empty((g.qx, g.qy))
        p[:, 0] = 5.0 + abs(grav)
        for j in range(1, g.qy):
            p[:, j] = p[:, j - 1] + 0.5 * g.dy * (rho[:, j - 1] + rho[:, j]) * grav
        rng = np.random.default_rng(seed)
        r = rng.random((4, g.qx, g.qy))
        rho = rho * (1.0 + amp * (2.0 * r[0] - 1.0))
        p = p * (1.0 + amp * (2.0 * r[1] - 1.0))
        u = amp * (2.0 * r[2] - 1.0)
        v = amp * (2.0 * r[3] - 1.0)
        if noise:
            n = np.random.default_rng(seed + 1000).random((4, g.qx, g.qy))
            rho, p = rho * (1.0 + noise * (2.0 * n[0] - 1.0)), p * (1.0 + noise * (2.0 * n[1] - 1.0))
            u, v = u * (1.0 + noise * (2.0 * n[2] - 1.0)), v * (1.0 + noise * (2.0 * n[3] - 1.0))
        dens[:, :] = rho
        xmom[:, :] = rho * u
        ymom[:, :] = rho * v
        ener[:, :] = p / (gamma - 1.0) + 0.5 * rho * (u * u + v * v)
    return init


def inputs(case, wb):
    nx, ny, sides, riemann, method, amp, extra = case
    d = {"mesh.nx": nx, "mesh.ny": ny, "compressible.limiter": 1, "compressible.grav": -1.0,
         "compressible.riemann": riemann, "compressible.temporal_method": method,
         "compressible.well_balanced": wb, "driver.tmax": 1.e3, "driver.max_steps": 1000000,
         "driver.verbose": 0, "vis.dovis": 0, "io.do_io": 0}
    d.update(sides)
    d.update(extra)
    return d


def make(case, seed, wb, amp=None, noise=0.0):
    p = Pyro("compressible_rk")
    p.add_problem("atmosphere", atmosphere(case[5] if amp is None else amp, seed, noise), problem_params={})
    p.initialize_problem("atmosphere", inputs_dict=inputs(case, wb))
    return p


def data(sim):
    return np.array(sim.cc_data.data)


def run(p, nsteps, capture=None):
    """nsteps single_steps; capture: dict that receives the first stage of the first step"""
    sim = p.sim
    dts = []
    for n in range(nsteps):
        if n == 0 and capture is not None:
            wcode, scode = reconstruction.well_balance.__code__, type(sim).substep.__code__

            def hook(frame, event, arg):
                if event != "return":
                    return
                if frame.f_code is wcode and "wb" not in capture:
                    capture["wb"] = np.array(arg)
                elif frame.f_code is scode and "k" not in capture:
                    capture["k"] = np.array(arg)
                    capture["U0"] = np.array(frame.f_locals["myd"].data)
            sys.setprofile(hook)
            try:
                p.single_step()
            finally:
                sys.setprofile(None)
        else:
            p.single_step()
        dts.append(sim.dt)
    return np.array(dts)


def interior_dev(a, b, ng):
    I = (slice(ng, -ng), slice(ng, -ng))
    scale = np.maximum(np.abs(b[I]).max(axis=(0, 1)), 1.e-3)    # (the floor of the tests: momenta at rest)
    return float((np.abs(a[I] - b[I]) / scale).max())


def comp_meta(sim):
    rp, g = sim.rp, sim.cc_data.grid
    return np.array([g.nx, g.ny, g.ng, g.dx, g.dy, rp.get_param("eos.gamma"),
                     rp.get_param("compressible.limiter"), rp.get_param("compressible.use_flattening"),
                     rp.get_param("compressible.z0"), rp.get_param("compressible.z1"),
                     rp.get_param("compressible.delta"), rp.get_param("compressible.cvisc"),
                     rp.get_param("compressible.grav"), rp.get_param("driver.cfl")])


def main():
    out = {"ncases": np.array(len(CASES))}
    for k, case in enumerate(CASES):
        seed = 500 + k
        pre = f"c{k}_"
        p = make(case, seed, 1)
        sim, rp = p.sim, p.sim.rp
        ng = sim.cc_data.grid.ng
        out[pre + "ic"] = data(sim)
        cap = {}
        out[pre + "dts"] = run(p, NSTEPS, cap)
        out[pre + "final"] = data(sim)
        assert np.all(np.isfinite(out[pre + "final"][ng:-ng, ng:-ng]))
        out[pre + "U0"], out[pre + "wb"], out[pre + "k"] = cap["U0"], cap["wb"], cap["k"]
        out[pre + "meta"] = comp_meta(sim)
        out[pre + "bc"] = np.array([rp.get_param(s) for s in SIDES])
        out[pre + "method"] = np.array(rp.get_param("compressible.temporal_method"))
        out[pre + "riemann"] = np.array(rp.get_param("compressible.riemann"))
        out[pre + "sponge"] = np.array([rp.get_param("sponge.do_sponge"), rp.get_param("sponge.sponge_rho_begin"),
                                        rp.get_param("sponge.sponge_rho_full"),
                                        rp.get_param("sponge.sponge_timescale")])
        out[pre + "drv"] = np.array([rp.get_param("driver.init_tstep_factor"),
                                     rp.get_param("driver.max_dt_change")])
        q = make(case, seed, 0)
        run(q, NSTEPS)
        plain = interior_dev(data(q.sim), out[pre + "final"], ng)
        t = make(case, seed, 1, noise=1.e-15)
        run(t, NSTEPS)
        twin = interior_dev(data(t.sim), out[pre + "final"], ng)
        out[pre + "plain_dev"], out[pre + "twin_dev"] = np.array(plain), np.array(twin)
        print(pre, case[0], case[1], case[3], case[4], "amp", case[5], "dts", out[pre + "dts"],
              "plain_dev %.2e twin_dev %.2e" % (plain, twin))
        assert plain > 1.e-6, (k, plain)
        assert twin <= 1.e-11, (k, twin)
    for k in REST_CASES:
        rest = []
        for wb in (1, 0):
            p = make(CASES[k], 0, wb, amp=0.0)
            run(p, NREST)
            ng = p.sim.cc_data.grid.ng
            rest.append(float(np.abs(data(p.sim)[ng:-ng, ng:-ng, 3]).max()))
        assert p.sim.ivars.iymom == 3
        out[f"rest{k}_wb"], out[f"rest{k}_plain"] = np.array(rest[0]), np.array(rest[1])
        print(f"rest{k}: max|ymom| after {NREST} steps: well-balanced %.2e plain %.2e" % tuple(rest))
        assert rest[0] <= 1.e-9 * rest[1], (k, rest)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "comp_rk_wb.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
