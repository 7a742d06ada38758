"""Buoyant bubble in an isothermal, hydrostatic atmosphere: the density falls off
exponentially with height, a disc of radius r_pert has its internal energy raised (and its
density lowered) at constant pressure.  The counterpart of the compressible solver's bubble
problem.  Reference: pyro/lm_atm/problems/bubble.py."""
import numpy as np

from ...util import msg

DEFAULT_INPUTS = "inputs.bubble"
PROBLEM_PARAMS = {"bubble.dens_base": 10.0,      # rho at y = 0
                  "bubble.scale_height": 2.0,    # e-folding height H of rho(y)
                  "bubble.x_pert": 2.0,
                  "bubble.y_pert": 2.0,
                  "bubble.r_pert": 0.25,
                  "bubble.pert_amplitude_factor": 5.0,
                  "bubble.dens_cutoff": 0.01}


def init_data(my_data, base, rp):
    """fill the state and the base state rho0 / p0 (objects with a .d array of qy values)"""
    if rp.get_param("driver.verbose"):
        msg.bold("initializing the bubble problem...")
    grav = rp.get_param("lm-atmosphere.grav")
    gamma = rp.get_param("eos.gamma")
    H = rp.get_param("bubble.scale_height")
    dens_base = rp.get_param("bubble.dens_base")
    dens_cutoff = rp.get_param("bubble.dens_cutoff")
    xp, yp, rpert = (rp.get_param("bubble." + k) for k in ("x_pert", "y_pert", "r_pert"))
    factor = rp.get_param("bubble.pert_amplitude_factor")

    g = my_data.grid
    dens = my_data.get_var("density")
    eint = my_data.get_var("eint")
    my_data.get_var("x-velocity")[:, :] = 0.0
    my_data.get_var("y-velocity")[:, :] = 0.0
    # stratified in y; the ghost rows keep the cutoff density (they enter the means below)
    dens[:, :] = dens_cutoff
    for j in range(g.jlo, g.jhi + 1):
        dens[:, j] = max(dens_base * np.exp(-g.y[j] / H), dens_cutoff)
    cs2 = H * abs(grav)
    pres = cs2 * dens
    eint[:, :] = pres / (gamma - 1.0) / dens
    # the bubble: more internal energy at the same pressure
    inside = np.sqrt((np.asarray(g.x2d) - xp)**2 + (np.asarray(g.y2d) - yp)**2) <= rpert
    eint[inside] = eint[inside] * factor
    dens[inside] = pres[inside] / (eint[inside] * (gamma - 1.0))
    # base state: horizontal means, then the pressure in hydrostatic equilibrium with rho0
    rho0, p0 = base["rho0"].d, base["p0"].d
    rho0[:] = np.mean(dens, axis=0)
    p0[:] = np.mean(pres, axis=0)
    for j in range(g.jlo + 1, g.jhi):
        p0[j] = p0[j - 1] + 0.5 * g.dy * (rho0[j] + rho0[j - 1]) * grav


def finalize():
    pass
