"""Fourth-order compressible solver (McCorquodale & Colella 2011: limited 4th-order face
states, CGF Riemann problems on primitive states, artificial viscosity) with Runge-Kutta
time integration; `Simulation` has the surface of pyro.compressible_fv4.Simulation.  The
right-hand side is one launch of csrc/comp_fv4.hip (k_fv4_rhs), the stage algebra
pyrohip_state_lincomb."""
from .simulation import Simulation

__all__ = ["Simulation"]
