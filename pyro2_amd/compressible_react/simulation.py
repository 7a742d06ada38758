"""compressible_react.Simulation with the call surface of
pyro/compressible_react/simulation.py: compressible.Simulation with the passive scalars "fuel"
and "ash" behind the four hydro variables (one launch of the tile kernel per step),
Strang-split around the reference's empty burn() / diffuse()."""
import numpy as np

from .. import compressible


class Simulation(compressible.Simulation):

    def initialize(self, *, extra_vars=None, ng=4):
        super().initialize(extra_vars=["fuel", "ash"] + list(extra_vars or []), ng=ng)

    def burn(self, dt):
        """react fuel to ash: nothing yet, as in the reference (simulation.py:20-27)"""

    def diffuse(self, dt):
        """thermal diffusion: nothing yet, as in the reference (simulation.py:29-36)"""

    def _advance_particles_by(self, dt):
        full = self.dt
        self.dt = dt
        try:
            self.advance_particles()
        finally:
            self.dt = full

    def evolve(self):
        """the reference's order (simulation.py:38-62), tracer quirk included: the particles
        advance dt/2 here, dt inside the hydro step and dt/2 after it -- 2 dt per step"""
        self.burn(self.dt / 2)
        self.diffuse(self.dt / 2)
        self._advance_particles_by(self.dt / 2)
        super().evolve()             # (advances t and n)
        self._advance_particles_by(self.dt / 2)
        self.diffuse(self.dt / 2)
        self.burn(self.dt / 2)

    def dovis(self):
        import matplotlib.pyplot as plt
        plt.clf()
        cc, g = self.cc_data, self.cc_data.grid
        ivars = compressible.Variables(cc)
        gamma = cc.get_aux("gamma")
        q = compressible.cons_to_prim(cc.data, gamma, ivars, g)
        rho, u, v, p = (q[:, :, n] for n in (ivars.irho, ivars.iu, ivars.iv, ivars.ip))
        fields = [rho, np.sqrt(u**2 + v**2), p, p / ((gamma - 1.0) * rho), q[:, :, ivars.ix]]
        names = [r"$\rho$", "U", "p", "e", r"$X_\mathrm{fuel}$"]
        for n, (f, nm) in enumerate(zip(fields, names)):
            ax = plt.subplot(2, 3, n + 1)
            img = ax.imshow(np.transpose(f[g.ilo:g.ihi + 1, g.jlo:g.jhi + 1]), interpolation="nearest",
                            origin="lower", extent=[g.xmin, g.xmax, g.ymin, g.ymax], cmap=self.cm)
            ax.set_title(nm)
            plt.colorbar(img, ax=ax)
        plt.figtext(0.05, 0.0125, f"t = {cc.t:10.5g}")
        plt.pause(0.001)
        plt.draw()
