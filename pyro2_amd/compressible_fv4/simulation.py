"""compressible_fv4.Simulation with the call surface of
pyro/compressible_fv4/simulation.py:9-80: the compressible_rk driver (stage by stage through
RKIntegrator) with the fourth-order right-hand side of McCorquodale & Colella.  Per stage:
ghost fill, pyrohip_comp_fv4_rhs (density floor, averages -> centres, primitives, flattening,
limited 4th-order face states, CGF on primitive states, face-centred fluxes, artificial
viscosity, sources at centres brought back to averages, sponge) -- one launch of the tile
kernel behind a light check launch; the stage starts and the final update are
pyrohip_state_lincomb launches.  The data are cell averages (mesh/fv.py FV2d).  Batches of
steps run on the device without a host round trip per stage (evolve_many:
pyrohip_comp_fv4_evolve)."""
from .. import device
from ..compressible_rk.simulation import Simulation as RKSimulation
from ..mesh import fv
from ..mesh import integration
from ..mesh import patch
from ..util import msg


class Simulation(RKSimulation):
    spherical_ok = False   # compressible_fv4/fluxes.py has no geometry terms
    decomposable = False   # (every stage would need a 5-cell halo exchange: single domain)
    # the data of a restart file are averages already: preevolve is not run over them
    restart_skips_preevolve = True

    def __init__(self, solver_name, problem_name, problem_func, rp, *,
                 problem_finalize_func=None, problem_source_func=None,
                 timers=None, data_class=fv.FV2d):
        if data_class is patch.CellCenterData2d:
            data_class = fv.FV2d
        super().__init__(solver_name, problem_name, problem_func, rp,
                         problem_finalize_func=problem_finalize_func,
                         problem_source_func=problem_source_func,
                         timers=timers, data_class=data_class)

    def initialize(self, *, extra_vars=None, ng=4):
        if ng != 4:
            msg.fail("ERROR: compressible_fv4 runs with 4 ghost cells")
        if self._rp_opt("mesh.grid_type", "Cartesian2d") == "SphericalPolar":
            msg.fail("ERROR: compressible_fv4 has no SphericalPolar geometry terms")
        from .. import decomp
        if int(self._rp_opt("gpu.decompose", -1)) == 1 or decomp.active_decomposition(self.rp) is not None:
            msg.fail("ERROR: compressible_fv4 / compressible_sdc run on a single domain (one GPU)")
        if self._rp_opt("compressible.well_balanced", 0):     # (the reference's solver has no such option)
            msg.fail("ERROR: compressible.well_balanced is an option of compressible_rk only")
        super().initialize(extra_vars=extra_vars, ng=ng)
        if self._host_source():
            msg.fail("ERROR: compressible_fv4 carries gravity, the sponge and heating profiles "
                     "(heating_profile) on the device; a host-evaluated source_terms() is not supported")

    def _params(self):
        """the compressible parameters; the limiter and Riemann solver are fixed by the
        scheme (fluxes.py:100, :141-144), compressible_sdc's defaults carry no limiter"""
        rp, g = self.rp, self.cc_data.grid
        opt = self._rp_opt
        heat = self._heating()
        return device.make_comp_params(
            g.dx, g.dy, gamma=rp.get_param("eos.gamma"), limiter=2,
            use_flattening=rp.get_param("compressible.use_flattening"),
            z0=rp.get_param("compressible.z0"), z1=rp.get_param("compressible.z1"),
            delta=rp.get_param("compressible.delta"), cvisc=rp.get_param("compressible.cvisc"),
            grav=rp.get_param("compressible.grav"),
            small_dens=rp.get_param("compressible.small_dens"),
            fast_math=opt("gpu.fast_math", 1), kernel_set=opt("gpu.kernel_set", -1),
            riemann="CGF", solid_xl=self.solid.xl, solid_yl=self.solid.yl,
            sponge=(rp.get_param("sponge.sponge_rho_begin"), rp.get_param("sponge.sponge_rho_full"),
                    rp.get_param("sponge.sponge_timescale"))
            if rp.get_param("sponge.do_sponge") else None,
            heat_rate=heat[0] if heat else 0.0)

    def substep(self, st, kstate, slot):
        """k of the cell-average device state `st` into slot `slot` of `kstate`"""
        st.comp_fv4_rhs(self._params(), kstate, slot)

    def preevolve(self):
        """the problem set up cell centres: convert them to averages (simulation.py:69-80)"""
        g = self.cc_data.grid
        if not abs(g.dx - g.dy) < 1.e-12 * g.dx:
            raise AssertionError("grid cells need to be square")
        for var in self.cc_data.names:
            self.cc_data.from_centers(var)

    def _rk_fusable(self, start, method):
        """the one-call Runge-Kutta step is compressible_rk's scheme: never for this one"""
        return False

    def _own_step(self):
        """the evolve / substep this class steps with: a subclass that replaces either steps singly"""
        return RKSimulation.evolve, Simulation.substep

    def can_evolve_many(self):
        """batches of steps on the device (pyrohip_comp_fv4_evolve): a single
        Cartesian domain with outflow / reflect / periodic sides and at least ng cells each way,
        gravity, the sponge and a heating profile included; no tracer set, nothing watching the
        data, no host-side boundary callback, the solver's own evolve and substep"""
        cc = self.cc_data
        if cc._views_alive() or self.particles is not None or cc.slab is not None:
            return False
        if getattr(self, "_device_stepping_refused", False):
            return False
        if (type(self).evolve, type(self).substep) != self._own_step():
            return False
        simple = ("outflow", "reflect-even", "reflect-odd", "periodic")
        if not all(b in simple for n in cc.names for b in cc.BCs[n].sides()):
            return False
        if any(cc._has_host_bc(n) for n in cc.names):
            return False
        g = cc.grid
        return g.nx >= g.ng and g.ny >= g.ng

    def _with_heating(self, states):
        """the heating profile on the states a right-hand side is taken of, as evolve() sets it"""
        h = self._heating()
        if h is not None:
            for st in states:
                if not getattr(st, "_heating_set", False):
                    st.set_heating(h[1])
                    st._heating_set = True

    def _loop_start(self):
        st = self._device_state()
        self.cc_data.take_pending_fill()     # (the loop fills the state's ghost cells itself)
        return st

    def evolve_many(self, nsteps):
        """up to nsteps of fill_BC_all + compute_timestep + evolve on the device: no host round
        trip per step or per stage.  Returns the time steps taken."""
        method = self.rp.get_param("compressible.temporal_method")
        nst = len(integration.b[method])

        def call(st, pol, cfl, n, particles):
            if self._rk_scratch is not None and self._rk_scratch[1].nvar != 4 * nst:
                self._rk_scratch = None
            rk = integration.RKIntegrator(self.cc_data.t, 0.0, method=method)
            self._rk_scratch = rk.set_start(st, self._rk_scratch)
            stage, k = self._rk_scratch
            self._with_heating([stage])
            return st.comp_fv4_evolve(self._params(), stage, k, integration.a[method], integration.b[method],
                                      cfl, pol, n, particles=particles)
        n0, entered = self.n, True
        try:
            dts = self._evolve_by_device_policy(nsteps, self._loop_start, call, refusable=True)
            entered = self.n > n0
            return dts
        finally:
            # evolve() asks for the fill of its first stage itself, and where fill_BC_all defers
            # fills that request outlives the step: the host then sees the new state's own images
            cc = self.cc_data
            if entered and cc.lazy_fill and cc._lazy_fill_ok():
                cc.fill_BC_all()
