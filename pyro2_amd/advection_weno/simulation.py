"""advection_weno.Simulation with the call surface of pyro/advection_weno/simulation.py:7-87:
advection_rk's driver with the WENO fluxes of advection_weno/fluxes.py
(pyrohip_advrk_params.scheme = 5)."""
import numpy as np

from ..advection_rk.simulation import Simulation as RKSimulation
from ..util import msg


class Simulation(RKSimulation):
    scheme = 5

    def _check_options(self):
        super()._check_options()
        order = self.rp.get_param("advection.weno_order")
        if order not in (2, 3):      # (advection_weno/fluxes.py:89: the reference's assert)
            msg.fail(f"ERROR: advection.weno_order = {order}: only 2 and 3 are implemented")
            raise ValueError(f"advection.weno_order {order!r} is not 2 or 3")

    def _params(self):
        p = super()._params()
        p.weno_order = int(self.rp.get_param("advection.weno_order"))
        u = self.rp.get_param("advection.u")
        v = self.rp.get_param("advection.v")
        p.alpha = float(np.sqrt(u**2 + v**2))        # advection_weno/fluxes.py:96, as written there
        return p
