"""burgers.Simulation with the call surface of pyro/burgers/simulation.py:
14-187.  evolve() = pyrohip_bg_step1: limited slopes, edge states, transverse
terms, Riemann/upwind fluxes and the conservative update in one launch
(csrc/burgers.hip; gpu.kernel_set = 0: the four staged launches of
pyrohip_bg_step, same bits).  The CFL step needs max|u|, max|v| over the whole
array: two device min/max reductions for a single step; a batch of steps
(evolve_many) takes them from the step kernel and never leaves the device
(pyrohip_bg_evolve)."""
import numpy as np

from ..mesh import patch
from ..simulation_null import NullSimulation, bc_setup, grid_setup


class Simulation(NullSimulation):
    def initialize(self):
        my_grid = grid_setup(self.rp, ng=4)
        my_data = patch.CellCenterData2d(my_grid)
        bc = bc_setup(self.rp)[0]
        my_data.register_var("x-velocity", bc)
        my_data.register_var("y-velocity", bc)
        my_data.create()
        self.cc_data = my_data
        self.setup_particles(bc)
        self.problem_func(self.cc_data, self.rp)

    def _max_abs(self, name):
        cc = self.cc_data
        lo, hi = cc.device_state().minmax(cc.names.index(name), buf=cc.grid.ng)
        return max(-lo, hi)

    def method_compute_timestep(self):
        """cfl * min(dx / max|u|, dy / max|v|) over the whole array
        (burgers/simulation.py:37-51)"""
        cfl = self.rp.get_param("driver.cfl")
        g = self.cc_data.grid
        xtmp = g.dx / max(self._max_abs("x-velocity"), self.SMALL)
        ytmp = g.dy / max(self._max_abs("y-velocity"), self.SMALL)
        self.dt = cfl * min(xtmp, ytmp)

    def evolve(self):
        tm = self.tc.timer("evolve")
        tm.begin()
        cc, g = self.cc_data, self.cc_data.grid
        st = cc.device_state()
        step = st.bg_step if self._rp_opt("gpu.kernel_set", -1) == 0 else st.bg_step1
        step(cc.names.index("x-velocity"), cc.names.index("y-velocity"), g.dx, g.dy,
             self.dt, self.rp.get_param("advection.limiter"))
        cc.device_modified()
        self.advance_particles()         # burgers/simulation.py:128-133 (updated u, v)
        cc.t += self.dt
        self.n += 1
        tm.end()

    def can_evolve_many(self):
        """batches of steps on the device (pyrohip_bg_evolve): standard boundary types filled
        by the device (there the step kernel's interior maxima are the whole-array maxima of
        method_compute_timestep), nothing watching the data, tracer particles only where the
        device advances them, the plain evolve() with the one-launch kernel"""
        cc = self.cc_data
        if cc._views_alive() or type(self).evolve is not Simulation.evolve:
            return False
        if self.particles is not None and self._device_particle_source() is None:
            return False
        simple = ("outflow", "reflect-even", "reflect-odd", "periodic")
        if not all(b in simple for n in cc.names for b in cc.BCs[n].sides()):
            return False
        if self._rp_opt("gpu.kernel_set", -1) == 0:
            return False
        return not any(cc._has_host_bc(n) for n in cc.names)

    def evolve_many(self, nsteps):
        rp, cc, g = self.rp, self.cc_data, self.cc_data.grid
        if cc.t >= self.tmax:
            # a finished run: the loop's first ghost fill would still replace the frame the last
            # step left (the boundary fill of the state before it)
            return np.empty(0)

        def start():
            st = cc.device_state()
            cc.take_pending_fill()
            return st
        return self._evolve_by_device_policy(
            nsteps, start, lambda st, pol, cfl, n, particles: st.bg_evolve(
                cc.names.index("x-velocity"), cc.names.index("y-velocity"), g.dx, g.dy,
                rp.get_param("advection.limiter"), cfl, pol, n, particles=particles))

    def dovis(self):
        import matplotlib.pyplot as plt
        plt.clf()
        g = self.cc_data.grid
        _, axes = plt.subplots(nrows=1, ncols=2, num=1, clear=True)
        for ax, name in zip(axes, ("x-velocity", "y-velocity")):
            img = ax.imshow(np.transpose(self.cc_data.get_var(name).v()), interpolation="nearest",
                            origin="lower", extent=[g.xmin, g.xmax, g.ymin, g.ymax], cmap=self.cm)
            ax.set_xlabel("x")
            ax.set_ylabel("y")
            ax.set_title(name)
            plt.colorbar(img, ax=ax)
        plt.figtext(0.05, 0.0125, f"t = {self.cc_data.t:10.5f}")
        plt.pause(0.001)
        plt.draw()
