"""2nd-order method-of-lines linear advection (piecewise-linear upwind fluxes, Runge-Kutta in
time); `Simulation` has the surface of pyro.advection_rk.Simulation, a step is one launch per
Runge-Kutta stage of csrc/advection_rk.hip."""
from .simulation import Simulation

__all__ = ["Simulation"]
