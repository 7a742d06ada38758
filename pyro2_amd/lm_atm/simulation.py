"""lm_atm.Simulation with the call surface of pyro/lm_atm/simulation.py:12-692.

One step (evolve, :286-618 of the reference) on the device:
  1. lm_mg_coeffs  eta = beta0^2 / rho on every multigrid level, from the density plane
     lm_mac_rhs    coeff = beta0 / rho, source = rho' g / rho, limited slopes, edge states with
                   transverse, coeff grad p and source terms, MAC velocities,
                   RHS div(beta0 U_MAC) of the MAC projection
  2. MG solve      rtol 1e-12, variable coefficients (csrc/multigrid.hip)
  3. lm_advect     MAC correction with the face-averaged beta0 / rho, rho edge states, density
                   update, eint, velocity edge states with 2 beta0 / (rho + rho_old), advective
                   terms, provisional velocities, buoyancy from rho_half, ghost fills
  4. lm_mg_coeffs from the new density; lm_proj_rhs: RHS div(beta0 U) / dt, guess = old phi
  5. MG solve
  6. lm_proj_update  phi, U -= dt (beta0 / rho) grad phi, grad p rule, ghost fills
The time step (max |u|, max |v|, the buoyancy bound) is reduced on the device as well; only
scalars come back.  The reference builds a new multigrid object for every solve; here one
device hierarchy per set of boundary types is kept and re-initialised.  One arithmetic only
(reference operation order, no contraction): there is no gpu.fast_math variant."""
import os

import numpy as np

from .. import device
from ..mesh import boundary as bnd
from ..mesh import patch
from ..simulation_null import NullSimulation, bc_setup, grid_setup
from ..util import msg

_PHI_BC = {"periodic": "periodic", "reflect": "neumann", "slipwall": "neumann",
           "outflow": "dirichlet"}
NAMES = ("density", "x-velocity", "y-velocity", "eint", "phi-MAC", "phi", "gradp_x", "gradp_y")


class Basestate:
    """a 1-d (y) array with ghost cells and the reference's views of it"""

    def __init__(self, ny, *, ng=0):
        self.ny, self.ng = ny, ng
        self.qy = ny + 2 * ng
        self.d = np.zeros(self.qy, dtype=np.float64)
        self.jlo, self.jhi = ng, ng + ny - 1

    def v(self, buf=0):
        return self.d[self.jlo - buf:self.jhi + 1 + buf]

    def v2d(self, buf=0):
        return self.d[np.newaxis, self.jlo - buf:self.jhi + 1 + buf]

    def v2dp(self, shift, buf=0):
        return self.d[np.newaxis, self.jlo + shift - buf:self.jhi + 1 + shift + buf]

    def jp(self, shift, buf=0):
        return self.d[self.jlo - buf + shift:self.jhi + 1 + buf + shift]


class Simulation(NullSimulation):
    # a restart takes all eight variables (grad p among them) from the file: the throw-away
    # step of preevolve must not run over them
    restart_skips_preevolve = True

    def __init__(self, solver_name, problem_name, problem_func, rp, *,
                 problem_finalize_func=None, problem_source_func=None, timers=None):
        super().__init__(solver_name, problem_name, problem_func, rp,
                         problem_finalize_func=problem_finalize_func,
                         problem_source_func=problem_source_func, timers=timers)
        self.base = {}
        self._aux_bcs = None
        self.in_preevolve = False
        self._mgs = {}
        self._base_on = None       # the DeviceState that holds the current base state
        self.mg_cycles = (0, 0)

    def initialize(self):
        # refusals (exceptions, so that a caller can tell them apart)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise ValueError("lm_atm is not domain-decomposed: WORLD_SIZE > 1, run it as one process")
        if self._opt("mesh.grid_type") == "SphericalPolar":
            raise ValueError("lm_atm has no SphericalPolar geometry terms (mesh.grid_type)")
        myg = grid_setup(self.rp, ng=4)
        if myg.nx != myg.ny or myg.nx < 2 or myg.nx & (myg.nx - 1):
            raise ValueError(f"lm_atm: the multigrid solver needs nx = ny = 2^n, not {myg.nx} x {myg.ny}")
        bc_dens, bc_xodd, bc_yodd = bc_setup(self.rp)
        my_data = patch.CellCenterData2d(myg)
        my_data.register_var("density", bc_dens)
        my_data.register_var("x-velocity", bc_xodd)
        my_data.register_var("y-velocity", bc_yodd)
        my_data.register_var("eint", bc_dens)      # a diagnostic
        # phi: Neumann where the velocity is given on the boundary (walls), Dirichlet at an
        # outflow (no tangential acceleration there)
        sides = []
        for k in ("xlboundary", "xrboundary", "ylboundary", "yrboundary"):
            b = self.rp.get_param("mesh." + k)
            if b not in _PHI_BC:
                msg.fail(f"ERROR: lm_atm: mesh.{k} = {b} has no boundary type for phi")
            sides.append(_PHI_BC[b])
        bc_phi = bnd.BC(xlb=sides[0], xrb=sides[1], ylb=sides[2], yrb=sides[3])
        my_data.register_var("phi-MAC", bc_phi)
        my_data.register_var("phi", bc_phi)
        my_data.register_var("gradp_x", bc_dens)
        my_data.register_var("gradp_y", bc_dens)
        my_data.create()
        self.cc_data = my_data
        assert tuple(my_data.names) == NAMES

        self._aux_bcs = (bc_dens, bc_yodd)      # of coeff and source_y (aux_data)

        self.base["rho0"] = Basestate(myg.ny, ng=myg.ng)
        self.base["p0"] = Basestate(myg.ny, ng=myg.ng)
        self.problem_func(self.cc_data, self.base, self.rp)

        gamma = self.rp.get_param("eos.gamma")
        self.base["beta0"] = Basestate(myg.ny, ng=myg.ng)
        self.base["beta0"].d[:] = self.base["p0"].d**(1.0 / gamma)
        # beta0 on the y edges; piecewise constant on the domain edges
        be = self.base["beta0-edges"] = Basestate(myg.ny, ng=myg.ng)
        be.jp(1)[:] = 0.5 * (self.base["beta0"].v() + self.base["beta0"].jp(1))
        be.d[myg.jlo] = self.base["beta0"].d[myg.jlo]
        be.d[myg.jhi + 1] = self.base["beta0"].d[myg.jhi]
        self._base_on = None

    @property
    def aux_data(self):
        """the reference's second patch (coeff, source_y).  Here the two are work planes of the
        device state: a snapshot of them as they stand now (after a step: 2 beta0 / (rho +
        rho_old) and the buoyancy from rho_half), downloaded on demand -- not inside a step"""
        if self._aux_bcs is None:
            return None
        aux = patch.CellCenterData2d(self.cc_data.grid)
        aux.register_var("coeff", self._aux_bcs[0])
        aux.register_var("source_y", self._aux_bcs[1])
        aux.create()
        st = self._state()
        aux.get_var("coeff")[:, :] = st.lm_stage("coeff")
        aux.get_var("source_y")[:, :] = st.lm_stage("source")
        return aux

    # ---- helpers ---------------------------------------------------------
    def make_prime(self, a, a0):
        return a - a0.v2d(buf=a0.ng)

    def _state(self):
        """the device state, with the base state on it"""
        st = self.cc_data.device_state()
        if self._base_on is not st:
            st.lm_set_base(self.base["rho0"].d, self.base["p0"].d, self.base["beta0"].d,
                           self.base["beta0-edges"].d)
            self._base_on = st
        return st

    def _mg(self, bcs):
        g = self.cc_data.grid
        key = tuple(bcs)
        if key not in self._mgs:
            self._mgs[key] = device.DeviceMG(self.cc_data.ctx, g.nx, xmin=g.xmin, xmax=g.xmax,
                                             ymin=g.ymin, ymax=g.ymax, bcs=list(bcs), alpha=0.0,
                                             beta=0.0, nsmooth=10, nsmooth_bottom=50)
        return self._mgs[key]

    # ---- reference surface --------------------------------------------------
    def method_compute_timestep(self):
        """min(cfl min(dx / max|u|, dy / max|v|), sqrt(2 dx / F_buoy)) with F_buoy =
        max |rho' g| / rho: the second bound carries the start from rest"""
        g = self.cc_data.grid
        cfl = self.rp.get_param("driver.cfl")
        grav = self.rp.get_param("lm-atmosphere.grav")
        out = self._state().lm_dt(g.dx, g.dy, cfl, grav)
        self.dt = out[0]
        if self.verbose > 0:      # the reference prints the advective bound alone here
            xtmp = g.dx / out[1] if out[3] != 0 else 1.e33
            ytmp = g.dy / out[2] if out[4] != 0 else 1.e33
            print(f"timestep is {cfl * min(xtmp, ytmp)}")

    def preevolve(self):
        """initial projection of the velocity field (rtol 1e-10), then one throw-away step
        whose grad p is kept (lm_atm/simulation.py:180-284)"""
        self.in_preevolve = True
        cc, g = self.cc_data, self.cc_data.grid
        for name in ("density", "x-velocity", "y-velocity"):
            cc.fill_BC(name)
        mg = self._mg(cc.BCs["phi"].sides())
        st = self._state()
        st.lm_mg_coeffs(mg)
        st.lm_proj_rhs(mg, g.dx, g.dy, 1.0, 0, 0)
        nc0 = mg.solve(rtol=1.e-10)[0]
        st.lm_proj_update(mg, g.dx, g.dy, 1.0, 0)
        cc.device_modified()
        orig = np.array(cc.data)                   # device -> host copy of the state
        self.method_compute_timestep()
        self.evolve()
        new = np.asarray(cc.data)
        igx, igy = cc.names.index("gradp_x"), cc.names.index("gradp_y")
        orig[:, :, igx] = new[:, :, igx]
        orig[:, :, igy] = new[:, :, igy]
        cc.data[:, :, :] = orig
        self.pre_cycles = (nc0,) + tuple(self.mg_cycles)
        if self.verbose > 0:
            print("done with the pre-evolution")
        self.in_preevolve = False

    def evolve(self):
        tm = self.tc.timer("evolve")
        tm.begin()
        cc, g = self.cc_data, self.cc_data.grid
        limiter = self.rp.get_param("lm-atmosphere.limiter")
        proj_type = self.rp.get_param("lm-atmosphere.proj_type")
        grav = self.rp.get_param("lm-atmosphere.grav")
        gamma = self.rp.get_param("eos.gamma")
        st = self._state()

        if self.verbose > 0:
            print("  making MAC velocities")
        mg = self._mg(cc.BCs["phi-MAC"].sides())
        st.lm_mg_coeffs(mg)
        st.lm_mac_rhs(mg, g.dx, g.dy, self.dt, limiter, grav)
        if self.verbose > 0:
            print("  MAC projection")
        nc1 = mg.solve(rtol=1.e-12)[0]
        if self.verbose > 0:
            print("  making u, v edge states")
            print("  doing provisional update of u, v")
        st.lm_advect(mg, g.dx, g.dy, self.dt, limiter, proj_type, grav, gamma)
        cc.device_modified()
        if self.verbose > 0:
            for name, lab in (("density", "rho"), ("x-velocity", "u  "), ("y-velocity", "v  ")):
                print(f"min/max {lab} = {cc.min(name)}, {cc.max(name)}")
            print("  final projection")
        st = self._state()
        mg = self._mg(cc.BCs["phi"].sides())
        st.lm_mg_coeffs(mg)
        st.lm_proj_rhs(mg, g.dx, g.dy, self.dt, 1, 1)
        nc2 = mg.solve(rtol=1.e-12)[0]
        st.lm_proj_update(mg, g.dx, g.dy, self.dt, proj_type)
        cc.device_modified()
        self.mg_cycles = (nc1, nc2)
        if not self.in_preevolve:
            cc.t += self.dt
            self.n += 1
        tm.end()

    def dovis(self):
        import matplotlib.pyplot as plt
        plt.clf()
        cc, g = self.cc_data, self.cc_data.grid
        rho = cc.get_var("density")
        u = cc.get_var("x-velocity")
        v = cc.get_var("y-velocity")
        rhoprime = self.make_prime(rho, self.base["rho0"])
        magvel = np.sqrt(u**2 + v**2)
        vort = g.scratch_array()
        vort.v()[:, :] = 0.5 * (v.ip(1) - v.ip(-1)) / g.dx - 0.5 * (u.jp(1) - u.jp(-1)) / g.dy
        _, axes = plt.subplots(nrows=2, ncols=2, num=1, clear=True)
        plt.subplots_adjust(hspace=0.25)
        for ax, f, name in zip(axes.flat, (rho, magvel, vort, rhoprime),
                               (r"$\rho$", r"|U|", r"$\nabla \times U$", r"$\rho'$")):
            img = ax.imshow(np.transpose(f.v()), interpolation="nearest", origin="lower",
                            extent=[g.xmin, g.xmax, g.ymin, g.ymax], cmap=self.cm)
            ax.set_xlabel("x")
            ax.set_ylabel("y")
            ax.set_title(name)
            plt.colorbar(img, ax=ax)
        plt.figtext(0.05, 0.0125, f"t = {cc.t:10.5f}")
        plt.pause(0.001)
        plt.draw()

    def write_extras(self, f):
        """the base state, as the group "base state" of the output file"""
        gb = f.create_group("base state")
        for name, state in self.base.items():
            gb.create_dataset(name, data=state.d)

    def read_extras(self, f):
        if "base state" not in f:
            return
        gb = f["base state"]
        g = self.cc_data.grid
        for name in gb:
            self.base[name] = Basestate(g.ny, ng=g.ng)
            self.base[name].d[:] = np.asarray(gb[name][...]).reshape(-1)
        self._base_on = None
