"""4th-order finite-volume linear advection (McCorquodale & Colella face states, Runge-Kutta in
time) on cell averages; `Simulation` has the surface of pyro.advection_fv4.Simulation, a step is
one launch per Runge-Kutta stage of csrc/advection_rk.hip."""
from .simulation import Simulation

__all__ = ["Simulation"]
