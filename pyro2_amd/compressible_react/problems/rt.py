"""Single-mode Rayleigh-Taylor instability with the two fluids tagged: the light fluid below
(dens1) is ash, the heavy one on top (dens2) is fuel, as partial densities (reference:
pyro/compressible_react/problems/rt.py -- its velocity perturbation is the plain cosine, not the
symmetrised one of the compressible solver's rt).  The shipped inputs.rt asks for hse sides, which
a run with passive scalars refuses: choose reflecting y sides to step it."""
import numpy as np

from ...util import msg

DEFAULT_INPUTS = "inputs.rt"
PROBLEM_PARAMS = {"rt.dens1": 1.0, "rt.dens2": 2.0, "rt.amp": 1.0,
                  "rt.sigma": 0.1, "rt.p0": 10.0}


def init_data(my_data, rp):
    msg.bold("initializing the rt problem...")
    gamma = rp.get_param("eos.gamma")
    grav = rp.get_param("compressible.grav")
    dens1, dens2 = rp.get_param("rt.dens1"), rp.get_param("rt.dens2")
    p0, amp, sigma = (rp.get_param("rt." + k) for k in ("p0", "amp", "sigma"))
    g = my_data.grid
    dens, ener = my_data.get_var("density"), my_data.get_var("energy")
    xmom, ymom = my_data.get_var("x-momentum"), my_data.get_var("y-momentum")
    fuel, ash = my_data.get_var("fuel"), my_data.get_var("ash")

    # stratification on the interior rows (all columns); ghost rows stay 0 until the first fill
    ymid = 0.5 * (g.ymin + g.ymax)
    y = np.asarray(g.y)
    inside = np.zeros(g.qy, dtype=bool)
    inside[g.jlo:g.jhi + 1] = True
    lower = inside & (y < ymid)
    upper = inside & ~(y < ymid)
    p_y = np.where(lower, p0 + dens1 * grav * y,
                   np.where(upper, p0 + dens1 * grav * ymid + dens2 * grav * (y - ymid), 0.0))
    ash[:, :] = np.where(lower, dens1, 0.0)[np.newaxis, :]
    fuel[:, :] = np.where(upper, dens2, 0.0)[np.newaxis, :]
    dens[:, :] = np.where(lower, dens1, np.where(upper, dens2, 0.0))[np.newaxis, :]

    x2d, y2d = np.asarray(g.x2d), np.asarray(g.y2d)
    xmom[:, :] = 0.0
    ymom[:, :] = amp * np.cos(2.0 * np.pi * x2d / (g.xmax - g.xmin)) * np.exp(-(y2d - ymid)**2 / sigma**2)
    ymom *= dens
    with np.errstate(invalid="ignore", divide="ignore"):   # 0/0 in the y ghost rows
        ener[:, :] = p_y[np.newaxis, :] / (gamma - 1.0) + 0.5 * (xmom**2 + ymom**2) / dens


def finalize():
    pass
