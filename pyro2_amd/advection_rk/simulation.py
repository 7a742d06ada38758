"""advection_rk.Simulation with the call surface of pyro/advection_rk/simulation.py:8-90: the
advection solver's state and problems with a method-of-lines update.  evolve() is one
pyrohip_advrk_step: one launch of the tile kernel of csrc/advection_rk.hip per Runge-Kutta
stage -- the stage start is formed and ghost-filled as the tile is loaded, the last stage writes
the final update -- instead of a linear combination, a ghost fill and a right-hand side each.
A subclass that overrides substep() or evolve() goes stage by stage through
mesh/integration.py's RKIntegrator (pyrohip_state_lincomb + pyrohip_advrk_rhs)."""
import numpy as np

from .. import _lib
from ..advection.simulation import Simulation as AdvectionSimulation
from ..mesh import integration
from ..simulation_null import bc_setup, grid_setup
from ..util import msg


class Simulation(AdvectionSimulation):
    scheme = 2          # pyrohip_advrk_params.scheme: the second-order fluxes

    def initialize(self):
        """grid (ng = 4), the single variable "density" in this solver's data class, then the
        problem's initial condition"""
        from .. import decomp
        if int(self._rp_opt("gpu.decompose", -1)) == 1 or decomp.active_decomposition(self.rp) is not None:
            msg.fail(f"ERROR: {self.solver_name} runs on a single domain (one GPU), not on a decomposed grid")
            raise ValueError(f"{self.solver_name} runs on a single domain")
        self._check_options()
        my_grid = grid_setup(self.rp, ng=4)
        my_data = self.data_class(my_grid)
        bc = bc_setup(self.rp)[0]
        my_data.register_var("density", bc)
        my_data.create()
        # the stage kernel takes ghost cells through the boundary rules: the driver's
        # fill_BC_all() is deferred into it
        my_data.lazy_fill = True
        self.cc_data = my_data
        self.setup_particles(bc)
        self.problem_func(self.cc_data, self.rp)
        self._rk_scratch = None

    def _check_options(self):
        """what does not run in the reference is refused, not given a meaning"""
        lim = int(self.rp.get_param("advection.limiter"))
        if self.scheme == 2 and lim >= 10:
            # (advection_rk/fluxes.py:72: reconstruction.limit returns one array, two are unpacked)
            msg.fail("ERROR: advection.limiter >= 10 does not run in the reference's advection_rk")
            raise ValueError("advection.limiter >= 10 is not supported by advection_rk")
        method = self.rp.get_param("advection.temporal_method")
        if method not in _lib.RK_METHODS:
            msg.fail(f"ERROR: advection.temporal_method = {method} is not one of {sorted(_lib.RK_METHODS)}")
            raise ValueError(f"unknown advection.temporal_method {method!r}")

    def _params(self):
        g = self.cc_data.grid
        return _lib.AdvRkParams(g.dx, g.dy, float(self.rp.get_param("advection.u")),
                                float(self.rp.get_param("advection.v")),
                                int(self.rp.get_param("advection.limiter")), self.scheme,
                                self._fast_math())

    def method_compute_timestep(self):
        """cfl / (max(|u|, SMALL) / dx + max(|v|, SMALL) / dy): closed form, nothing to reduce
        (advection_rk/simulation.py:31-47; not the parent's minimum over the directions)"""
        cfl = self.rp.get_param("driver.cfl")
        u = self.rp.get_param("advection.u")
        v = self.rp.get_param("advection.v")
        g = self.cc_data.grid
        xtmp = max(abs(u), self.SMALL) / g.dx
        ytmp = max(abs(v), self.SMALL) / g.dy
        self.dt = cfl / (xtmp + ytmp)

    def substep(self, st, kstate, slot):
        """k = -div F of the device state `st` (ghost cells through the boundary rules) into
        slot `slot` of `kstate`"""
        st.advrk_rhs(self.cc_data.names.index("density"), self._params(), kstate, slot)

    def _fused(self):
        """the one-call step is this class's scheme: a subclass with its own substep() goes
        stage by stage; so does a boundary the kernel does not take through its index maps"""
        cc = self.cc_data
        if type(self).substep is not Simulation.substep or cc.slab is not None:
            return False
        simple = ("outflow", "reflect-even", "periodic")
        if not all(b in simple for n in cc.names for b in cc.BCs[n].sides()):
            return False
        return not any(cc._has_host_bc(n) for n in cc.names)

    def _after_step(self):
        if self.particles is not None:   # constant velocity field, advection_rk/simulation.py:73-81
            g = self.cc_data.grid
            self.advance_particles(g.scratch_array() + self.rp.get_param("advection.u"),
                                   g.scratch_array() + self.rp.get_param("advection.v"))
        self.cc_data.t += self.dt
        self.n += 1

    def evolve(self):
        """one Runge-Kutta step of "density" on the device"""
        tm = self.tc.timer("evolve")
        tm.begin()
        cc = self.cc_data
        method = self.rp.get_param("advection.temporal_method")
        if self._fused():
            st = cc.device_state(fuse_fill=True)
            cc.take_pending_fill()               # every stage applies the boundary rules itself
            st.advrk_step(cc.names.index("density"), self._params(), method, float(self.dt))
        else:
            self._evolve_staged(method)
        cc.device_modified()
        self._after_step()
        tm.end()

    def _evolve_staged(self, method):
        """advection_rk/simulation.py:60-71 with RKIntegrator on device states"""
        cc = self.cc_data
        start = cc.device_state()            # (a deferred ghost fill is carried out)
        rk = integration.RKIntegrator(cc.t, self.dt, method=method)
        if self._rk_scratch is not None and self._rk_scratch[1].nvar != cc.nvar * rk.nstages():
            self._rk_scratch = None
        self._rk_scratch = rk.set_start(start, self._rk_scratch)
        for s in range(rk.nstages()):
            ytmp = rk.get_stage_start(s)
            ytmp.fill_bc(-1)                 # (stage 0: the state's own ghost cells, as the reference)
            self.substep(ytmp, rk.k, s)
            rk.store_increment(s)
        rk.compute_final_update()

    def can_evolve_many(self):
        """may the driver hand several steps at once to the device (pyrohip_advrk_evolve)?
        The plain evolve() and substep() of this class, nothing watching the data (tracer
        particles ride along: the velocity is constant, they never read the data)."""
        cc = self.cc_data
        if type(self).evolve is not Simulation.evolve or not self._fused():
            return False
        return not cc._views_alive()

    def evolve_many(self, nsteps):
        """up to nsteps iterations of fill_BC_all + compute_timestep + evolve in one device
        call: the time step is closed-form, so the driver's policy gives the whole dt sequence
        beforehand -- computed here by the very methods the single step uses.  Returns the
        time steps taken."""
        tm = self.tc.timer("evolve")
        tm.begin()
        cc = self.cc_data
        dts = self._plan_timesteps(nsteps, lambda dt: dt > 0.0 and np.isfinite(dt))
        if dts:
            st = cc.device_state(fuse_fill=True)
            cc.take_pending_fill()
            try:
                st.advrk_evolve(cc.names.index("density"), self._params(),
                                self.rp.get_param("advection.temporal_method"), dts)
            finally:
                cc.device_modified()
            for dt in dts:                       # the same additions in the same order
                self.dt = dt
                self._after_step()
        tm.end()
        return dts
