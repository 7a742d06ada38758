"""compressible_sdc.Simulation with the call surface of
pyro/compressible_sdc/simulation.py:9-127.  One step = 9 right-hand sides
(pyrohip_comp_fv4_rhs) and 8 node updates (pyrohip_comp_sdc_update, each followed by a
ghost fill).  The advective terms A of the nodes are slots of one device k-state: the old
and new iterations swap slots instead of copying.  Batches of steps run on the device without a
host round trip per right-hand side (evolve_many: pyrohip_comp_sdc_evolve)."""
from .. import device
from ..compressible_fv4.simulation import Simulation as FV4Simulation
from ..util import msg

# sdc_integral (simulation.py:20-36): dt/24 (c0 A_0 + c1 A_1 + c2 A_2) from node m to m + 1
_SDC_C = ((5.0, 8.0, -1.0), (-1.0, 8.0, 5.0))


class Simulation(FV4Simulation):
    """the 4th-order compressible solver with SDC time integration"""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.n_nodes = 3  # Gauss-Lobatto temporal nodes
        self.n_iter = 4   # 4 SDC iterations for 4th order
        self._sdc_scratch = None

    def _scratch(self, start):
        """the states of nodes 1 and 2 and a k-state of 5 slots (A_old[0] = A_new[0], and two
        generations of A_1, A_2)"""
        if self._sdc_scratch is None:
            rows = [list(r) for r in start.bc]
            nodes = [device.DeviceState(start.ctx, start.nx, start.ny, start.ng, rows) for _ in range(2)]
            k = device.DeviceState(start.ctx, start.nx, start.ny, start.ng, [["outflow"] * 4] * (4 * 5))
            self._sdc_scratch = (nodes, k)
        return self._sdc_scratch

    def evolve(self):
        """one step of compressible_sdc/simulation.py:48-127"""
        tm = self.tc.timer("evolve")
        tm.begin()
        cc = self.cc_data
        dt = float(self.dt)
        start = self._device_state()            # node 0 (ghost cells filled by the driver)
        (n1, n2), k = self._scratch(start)
        h = self._heating()
        if h is not None:
            for st in (n1, n2):
                if not getattr(st, "_heating_set", False):
                    st.set_heating(h[1])
                    st._heating_set = True
        U = [start, n1, n2]
        self.substep(start, k, 0)
        old = [0, 0, 0]                        # A_kold[m] -> slot
        for _ in range(self.n_iter):
            free = [s for s in range(1, 5) if s not in old]
            new = [0, None, None]
            for m in range(self.n_nodes):
                if m > 0:
                    new[m] = free.pop(0)
                    self.substep(U[m], k, new[m])
                if m < self.n_nodes - 1:
                    U[m + 1].comp_sdc_update(U[m], k, new[m], old[m], old, _SDC_C[m], dt)
                    cc._push_user_bc(U[m + 1])
                    U[m + 1].fill_bc(-1)
            old = [0, new[1], new[2]]
        start.lincomb(n2, k, [])                # the new solution, ghost cells included
        cc.device_modified()
        self.advance_particles()
        cc.t += self.dt
        self.n += 1
        tm.end()

    def _own_step(self):
        return Simulation.evolve, FV4Simulation.substep

    def evolve_many(self, nsteps):
        """up to nsteps of fill_BC_all + compute_timestep + evolve on the device
        (pyrohip_comp_sdc_evolve): the 9 right-hand sides and 8 node updates of every step without a
        host round trip.  Returns the time steps taken."""
        def call(st, pol, cfl, n, particles):
            (n1, n2), k = self._scratch(st)
            self._with_heating([n1, n2])
            return st.comp_sdc_evolve(self._params(), n1, n2, k, cfl, pol, n, particles=particles)
        return self._evolve_by_device_policy(nsteps, self._loop_start, call, refusable=True)

    def sdc_integral(self, m_start, m_end, As):
        """host form of the quadrature (analysis; the step runs pyrohip_comp_sdc_update)"""
        if (m_start, m_end) not in ((0, 1), (1, 2)):
            msg.fail("invalid quadrature range")
        c = _SDC_C[m_start]
        integral = self.cc_data.grid.scratch_array(nvar=self.ivars.nvar)
        for n in range(self.ivars.nvar):
            integral.v(n=n)[:, :] = self.dt / 24.0 * (c[0] * As[0].v(n=n) + c[1] * As[1].v(n=n) +
                                                       c[2] * As[2].v(n=n))
        return integral
