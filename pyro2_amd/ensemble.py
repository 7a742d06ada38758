#!/usr/bin/env python3
"""An ensemble: N independent small `compressible` runs stepped together.

A 64^2 grid is 15 workgroups of the tile kernel on a card that keeps 512 resident: a parameter
study of such runs, taken one after the other, pays the launch floor N times per step.  Here
the members -- same grid, boundary types and solver parameters, their own data, dt sequence,
time and last step -- advance in two launches per step for all of them:

    ens = Ensemble("compressible")
    for r in (0.01, 0.02, 0.04):
        ens.add("sedov", "inputs.sedov", {"sedov.r_init": r})
    ens.run_sim()
    for p in ens.members:
        print(p.sim.cc_data.t, p.sim.n)        # ... p.sim.write(name)

Every member is an ordinary `Pyro`; after run_sim() its `sim` is as after its own
`Pyro.run_sim()` (bit for bit with gpu.fast_math = 0).  Nothing is written or plotted while
the ensemble runs.  Meant for small grids: above about 1024^2 a single run is the better tool.

Command line:  python -m pyro2_amd.ensemble compressible sedov inputs.sedov \\
                   --vary sedov.r_init=0.01,0.02,0.04 [section.option=value ...]
"""
import argparse

from . import device
from .pyro_sim import Pyro
from .util import msg
from .util.runparams import _get_val


class Ensemble:
    def __init__(self, solver_name="compressible"):
        self.solver_name = solver_name
        self.members = []

    def add(self, problem_name, inputs_file=None, inputs_dict=None):
        """a member: an ordinary Pyro for this problem, initialised as usual; returned"""
        p = Pyro(self.solver_name)
        p.initialize_problem(problem_name, inputs_file=inputs_file, inputs_dict=inputs_dict)
        self.members.append(p)
        return p

    # ---- what members must share ------------------------------------------------------
    def _check(self):
        if self.solver_name != "compressible":
            msg.fail(f"ERROR: ensemble: solver {self.solver_name}: an ensemble steps the compressible solver only "
                     "(the method-of-lines solvers, swe and burgers are not carried)")
        if not self.members:
            msg.fail("ERROR: ensemble: no members (Ensemble.add)")
        first = self.members[0]
        g0 = first.sim.cc_data.grid
        sides0 = [tuple(first.sim.cc_data.BCs[n].sides()) for n in first.sim.cc_data.names]
        p0 = bytes(first.sim._params())
        for k, p in enumerate(self.members):
            sim, rp = p.sim, p.rp
            who = f"ERROR: ensemble: member {k}: "
            if p.solver_name != "compressible":
                msg.fail(who + f"solver {p.solver_name}: every member runs the compressible solver")
            if rp.get_param("io.do_io") or rp.get_param("vis.dovis"):
                opt = "io.do_io" if rp.get_param("io.do_io") else "vis.dovis"
                msg.fail(who + f"{opt} must be 0: nothing is written or plotted while the ensemble runs "
                               "(write members out with sim.write() afterwards)")
            if sim.particles is not None:
                msg.fail(who + "tracer particles (particles.do_particles) are not carried in an ensemble")
            if not sim.can_evolve_many():
                msg.fail(who + "can_evolve_many() is False: the run cannot step on the device in batches "
                               "(host-evaluated sources, passive scalars, gpu.kernel_set = 0, host-side boundaries)")
            g = sim.cc_data.grid
            for opt, a, b in (("mesh.nx", g.nx, g0.nx), ("mesh.ny", g.ny, g0.ny), ("mesh ng", g.ng, g0.ng),
                              ("mesh.grid_type", g.coord_type, g0.coord_type),
                              ("mesh.xmin", g.xmin, g0.xmin), ("mesh.xmax", g.xmax, g0.xmax),
                              ("mesh.ymin", g.ymin, g0.ymin), ("mesh.ymax", g.ymax, g0.ymax)):
                if a != b:
                    msg.fail(who + f"{opt} = {a} differs from member 0's ({b}): one grid for all members")
            sides = [tuple(sim.cc_data.BCs[n].sides()) for n in sim.cc_data.names]
            if sides != sides0:
                names = ("mesh.xlboundary", "mesh.xrboundary", "mesh.ylboundary", "mesh.yrboundary")
                bad = next(names[s] for a, b in zip(sides, sides0) for s in range(4) if a[s] != b[s])
                msg.fail(who + f"{bad} differs from member 0's: one set of boundary types for all members")
            if float(rp.get_param("driver.cfl")) != float(first.rp.get_param("driver.cfl")):
                msg.fail(who + f"driver.cfl = {rp.get_param('driver.cfl')} differs from member 0's")
            P = sim._params()
            if bytes(P) != p0:
                P0 = first.sim._params()
                bad = next(f for f, _ in P._fields_ if getattr(P, f) != getattr(P0, f))
                msg.fail(who + f"solver parameter {bad} = {getattr(P, bad)} differs from member 0's "
                               f"({getattr(P0, bad)}): members differ in their data only")

    # ---- running ----------------------------------------------------------------------
    def run_sim(self):
        """every member to its own driver.tmax / driver.max_steps, in batches of steps on the
        device; t, n, dt, dt_old go back into every member's sim"""
        from .decomp import DtPolicy
        self._check()
        running = [p for p in self.members if not p.sim.finished()]
        while running:
            sims = [p.sim for p in running]
            # the batch length as Pyro.run_sim hands it to evolve_many, the smallest over the members
            nsteps = min(min(getattr(s, "batch_steps", 64), s.max_steps - s.n) for s in sims)
            pols = []
            for s in sims:
                rp = s.rp
                pol = DtPolicy(s.tmax, rp.get_param("driver.init_tstep_factor"),
                               rp.get_param("driver.max_dt_change"), rp.get_param("driver.fix_dt"))
                pol.t, pol.n = float(s.cc_data.t), int(s.n)
                pol.dt_old = float(getattr(s, "dt_old", -1.e33))
                pols.append(pol)
            states = [s._device_state() for s in sims]
            err = None
            try:
                dts, _ = device.DeviceState.comp_evolve_batch(states, sims[0]._params(),
                                                              float(sims[0].rp.get_param("driver.cfl")), pols, nsteps)
            except device._lib.PyroHipError as e:
                if not hasattr(e, "all_dts"):      # a refusal: nothing ran
                    raise
                err, dts = e, e.all_dts
            finally:
                for s in sims:
                    s.cc_data.device_modified()
            for s, pol, d in zip(sims, pols, dts):
                s.cc_data.t, s.n, s.dt_old = pol.t, pol.n, pol.dt_old
                if len(d):
                    s.dt = float(d[-1])
            if err is not None:     # a member met an invalid state: the others stand where this batch left them
                raise err
            if not any(len(d) for d in dts):
                msg.fail("ERROR: ensemble: no member advanced (a zero time step)")
            running = [p for p in running if not p.sim.finished()]
        return self.members


def main(argv=None):
    ap = argparse.ArgumentParser(description="step an ensemble of small compressible runs together")
    ap.add_argument("solver", metavar="solver-name")
    ap.add_argument("problem", metavar="problem-name")
    ap.add_argument("param", metavar="inputs-file")
    ap.add_argument("--vary", action="append", default=[], metavar="section.option=v1,v2,...",
                    help="one member per value (several --vary: their values member by member)")
    ap.add_argument("other", metavar="runtime-parameters", nargs="*", help="section.option=value overrides")
    args = ap.parse_intermixed_args(argv)
    common = dict((k, _get_val(v)) for k, v in (item.split("=") for item in args.other))
    varied = [(k, [_get_val(x) for x in v.split(",")]) for k, v in (item.split("=") for item in args.vary)]
    if not varied or len({len(v) for _, v in varied}) != 1:
        msg.fail("ERROR: ensemble: --vary section.option=v1,v2,... (the same number of values in each)")
    ens = Ensemble(args.solver)
    for m in range(len(varied[0][1])):
        d = {"io.do_io": 0, "vis.dovis": 0, "driver.verbose": 0}
        d.update(common)
        d.update({k: v[m] for k, v in varied})
        ens.add(args.problem, args.param, d)
    ens.run_sim()
    for m, p in enumerate(ens.members):
        what = " ".join(f"{k}={v[m]}" for k, v in varied)
        print("member %d %s: t = %.8g n = %d dt = %.8g" % (m, what, p.sim.cc_data.t, p.sim.n, p.sim.dt))
    return ens


if __name__ == "__main__":
    main()
