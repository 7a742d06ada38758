"""compressible_fv4.Simulation with the call surface of
pyro/compressible_fv4/simulation.py:9-80: the compressible_rk driver (stage by stage through
RKIntegrator) with the fourth-order right-hand side of McCorquodale & Colella.  Per stage:
ghost fill, pyrohip_comp_fv4_rhs (density floor, averages -> centres, primitives, flattening,
limited 4th-order face states, CGF on primitive states, face-centred fluxes, artificial
viscosity, sources at centres brought back to averages, sponge) -- one launch of the tile
kernel behind a light check launch; the stage starts and the final update are
pyrohip_state_lincomb launches.  The data are cell averages (mesh/fv.py FV2d)."""
from .. import device
from ..compressible_rk.simulation import Simulation as RKSimulation
from ..mesh import fv
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

    def can_evolve_many(self):
        return False
