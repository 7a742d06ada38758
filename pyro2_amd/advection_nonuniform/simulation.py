"""advection_nonuniform.Simulation with the call surface of
pyro/advection_nonuniform/simulation.py:11-164; evolve() is one launch of the LDS-tiled
kernel of csrc/advection_nonuniform.hip (pyrohip_advnu_step)."""
import numpy as np

from ..mesh import patch
from ..mesh.array_indexer import ArrayIndexer
from ..simulation_null import NullSimulation, bc_setup, grid_setup


def upwind_shift(velocity):
    """-1 where the velocity is positive, 0 elsewhere: the offset of the cell a face's state
    is taken from (advection_nonuniform/simulation.py:18-26)"""
    return np.where(np.asarray(velocity) > 0, -1.0, 0.0)


class Simulation(NullSimulation):
    # steps the driver hands over at once when it batches
    batch_steps = 96

    def initialize(self):
        """grid (ng = 4), the five variables in the reference's order, the problem's initial
        condition, then the upwind shifts of the velocity field it set"""
        # (not decomposable: under a launcher every process runs the whole problem)
        my_grid = grid_setup(self.rp, ng=4)
        bc, bc_xodd, bc_yodd = bc_setup(self.rp)
        my_data = patch.CellCenterData2d(my_grid)
        my_data.register_var("x-velocity", bc_xodd)
        my_data.register_var("y-velocity", bc_yodd)
        my_data.register_var("x-shift", bc_xodd)
        my_data.register_var("y-shift", bc_yodd)
        my_data.register_var("density", bc)
        my_data.create()
        # the step kernel takes ghost cells through the boundary rules: the driver's
        # fill_BC_all() is deferred into it
        my_data.lazy_fill = True
        self.cc_data = my_data
        self.setup_particles(bc)
        self.problem_func(self.cc_data, self.rp)
        # on the host, stored with the output; the kernel derives the same offsets from the
        # signs of the velocities (csrc/advection_nonuniform.hip: contract)
        my_data.get_var("x-shift")[:, :] = upwind_shift(my_data.get_var("x-velocity"))
        my_data.get_var("y-shift")[:, :] = upwind_shift(my_data.get_var("y-velocity"))
        self._cfl_step = None     # (cfl, dt) of the velocity field on the device
        self._uv = None           # host copies of the filled velocity planes (particles)
        self._uploads = -1        # DeviceState.uploads when the two were taken

    def _ivars(self):
        names = self.cc_data.names
        return names.index("density"), names.index("x-velocity"), names.index("y-velocity")

    def _field_current(self):
        """the device copy is the data and is the one the cached quantities were taken from:
        nothing on the host has touched the velocities since"""
        cc = self.cc_data
        return cc._dev_valid and cc._dev is not None and cc._dev.uploads == self._uploads

    def method_compute_timestep(self):
        """cfl min(dx / max|u|, dy / max|v|), the maxima over the whole array with its ghost
        cells as the driver's fill left them; no floor: a direction without motion gives inf
        (advection_nonuniform/simulation.py:64-82).  The velocities do not change during a
        run: reduced on the device once, again after the host copy was handed out."""
        cfl = self.rp.get_param("driver.cfl")
        if self._cfl_step is None or self._cfl_step[0] != cfl or not self._field_current():
            g = self.cc_data.grid
            st = self.cc_data.device_state()      # (carries out a deferred ghost fill)
            _, iu, iv = self._ivars()
            self._cfl_step = (cfl, st.advnu_dt(iu, iv, g.dx, g.dy, cfl))
            self._uv, self._uploads = None, st.uploads
        self.dt = self._cfl_step[1]

    def _fast_math(self):
        """gpu.fast_math (default 1: the contracted build; 0: the bit-faithful audit build)"""
        try:
            return int(self.rp.get_param("gpu.fast_math"))
        except (KeyError, ValueError):
            return 1

    def _velocities(self):
        """the velocity arrays for the tracer particles, ghost cells filled: fetched from the
        device once"""
        if self._uv is None or not self._field_current():
            cc = self.cc_data
            st = cc.device_state()                # (carries out a deferred ghost fill)
            _, iu, iv = self._ivars()
            if st.uploads != self._uploads:
                self._cfl_step, self._uploads = None, st.uploads
            self._uv = tuple(ArrayIndexer(d=st.download_var(n), grid=cc.grid) for n in (iu, iv))
        return self._uv

    def evolve(self):
        """one time step of "density" on the device"""
        tm = self.tc.timer("evolve")
        tm.begin()
        cc = self.cc_data
        g = cc.grid
        uv = self._velocities() if self.particles is not None else None
        st = cc.device_state(fuse_fill=True)
        cc.take_pending_fill()                   # the kernel applies the boundary rules itself
        ia, iu, iv = self._ivars()
        st.advnu_step(ia, iu, iv, g.dx, g.dy, float(self.dt),
                      int(self.rp.get_param("advection.limiter")), fast_math=self._fast_math())
        cc.device_modified()
        if uv is not None:                       # advection_nonuniform/simulation.py:110-114
            self.advance_particles(*uv)
        cc.t += self.dt
        self.n += 1
        tm.end()

    def can_evolve_many(self):
        """may the driver hand several steps at once to the device (pyrohip_advnu_evolve)?
        Standard boundary types, nothing watching the data, the plain evolve() of this class
        (tracer particles ride along: the velocity field is constant)."""
        cc = self.cc_data
        if type(self).evolve is not Simulation.evolve or cc.slab is not None:
            return False
        simple = ("outflow", "reflect-even", "reflect-odd", "periodic")
        if not all(b in simple for n in cc.names for b in cc.BCs[n].sides()):
            return False
        return not (any(cc._has_host_bc(n) for n in cc.names) or cc._views_alive())

    def evolve_many(self, nsteps):
        """up to nsteps iterations of fill_BC_all + compute_timestep + evolve
        (pyro_sim.py:250-256) in one device call.  The velocities do not change, so the
        driver's policy (simulation_null.py:222-244) gives the whole dt sequence beforehand --
        computed here by the very methods the single step uses.  Returns the time steps taken."""
        tm = self.tc.timer("evolve")
        tm.begin()
        cc = self.cc_data
        cc.fill_BC_all()                         # (the time step looks at filled ghost cells)
        n0 = self.n
        dts = self._plan_timesteps(nsteps, lambda dt: dt > 0.0 and np.isfinite(dt))
        if dts:
            g = cc.grid
            uv = self._velocities() if self.particles is not None else None
            st = cc.device_state(fuse_fill=True)
            cc.take_pending_fill()               # every step of the call fills
            ia, iu, iv = self._ivars()
            try:
                st.advnu_evolve(ia, iu, iv, g.dx, g.dy, dts,
                                int(self.rp.get_param("advection.limiter")),
                                fast_math=self._fast_math())
            finally:
                cc.device_modified()
            for dt in dts:                       # the same additions in the same order
                if uv is not None:
                    self.dt = dt
                    self.advance_particles(*uv)
                cc.t += dt
            self.n = n0 + len(dts)
        tm.end()
        return dts

    def dovis(self):
        """runtime plot of the density and the tracer particles (same picture as the
        reference's dovis)"""
        import matplotlib.pyplot as plt
        plt.clf()
        dens = self.cc_data.get_var("density")
        g = self.cc_data.grid
        img = plt.imshow(np.transpose(dens.v()), interpolation="nearest", origin="lower",
                         extent=[g.xmin, g.xmax, g.ymin, g.ymax], cmap=self.cm)
        plt.xlabel("x")
        plt.ylabel("y")
        plt.colorbar(img)
        plt.title("density")
        if self.particles is not None:
            pos = self.particles.get_positions()
            plt.scatter(pos[:, 0], pos[:, 1], c=self.particles.get_init_positions()[:, 0], cmap="Greys")
            plt.xlim([g.xmin, g.xmax])
            plt.ylim([g.ymin, g.ymax])
        plt.figtext(0.05, 0.0125, f"t = {self.cc_data.t:10.5f}")
        plt.pause(0.001)
        plt.draw()
