"""Fourth-order compressible solver with 4th-order spectral deferred corrections in time
(3 Gauss-Lobatto nodes, 4 iterations); `Simulation` has the surface of
pyro.compressible_sdc.Simulation.  Right-hand sides: csrc/comp_fv4.hip; node updates:
pyrohip_comp_sdc_update."""
from .simulation import Simulation

__all__ = ["Simulation"]
