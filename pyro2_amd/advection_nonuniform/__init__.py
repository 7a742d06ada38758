"""2nd-order unsplit CTU linear advection in a velocity field that varies from cell to cell;
`Simulation` has the surface of pyro.advection_nonuniform.Simulation, the update runs in
csrc/advection_nonuniform.hip."""
from .simulation import Simulation

__all__ = ["Simulation"]
