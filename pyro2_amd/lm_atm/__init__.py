"""Low Mach number atmospheric solver: pseudo-incompressible flow in a stratified
background (rho0, p0, beta0 = p0^(1/gamma)); `Simulation` has the surface of
pyro.lm_atm.Simulation.  The density-carrying CTU predictor, the beta0-weighted
divergences and corrections and the buoyancy run in csrc/lm_atm.hip, the two
variable-coefficient elliptic solves per step in the V-cycle of csrc/multigrid.hip with
coefficients beta0^2 / rho built on the device; no field leaves HBM inside Pyro.run_sim."""
from .simulation import Basestate, Simulation

__all__ = ["Basestate", "Simulation"]
