"""Method-of-lines linear advection with WENO reconstructions (r = 2 or 3) of Lax-Friedrichs split
fluxes, Runge-Kutta in time; `Simulation` has the surface of pyro.advection_weno.Simulation, a
step is one launch per Runge-Kutta stage of csrc/advection_rk.hip."""
from .simulation import Simulation

__all__ = ["Simulation"]
