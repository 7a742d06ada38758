"""compressible with two passive scalars, "fuel" and "ash" (the surface of
pyro.compressible_react): the CTU step of the compressible solver carries their partial
densities; burning and diffusion are the reference's empty hooks around it."""
from .simulation import Simulation

__all__ = ["Simulation"]
