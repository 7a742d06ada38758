"""The "flame" problem of compressible_react: the Sedov blast of the compressible solver with
r_init = 0.1 and 4 x 4 sub-samples fixed in the code (the inputs file's sedov.r_init is not read,
as in the reference: pyro/compressible_react/problems/flame.py), fuel and ash left at zero."""
import math

import numpy as np

from ...util import msg

DEFAULT_INPUTS = "inputs.flame"
PROBLEM_PARAMS = {"sedov.r_init": 0.1}     # (inputs.flame sets the key; the code below does not read it)


def init_data(my_data, rp):
    msg.bold("initializing the flame problem...")
    g = my_data.grid
    gamma = rp.get_param("eos.gamma")
    xctr = 0.5 * (rp.get_param("mesh.xmin") + rp.get_param("mesh.xmax"))
    yctr = 0.5 * (rp.get_param("mesh.ymin") + rp.get_param("mesh.ymax"))
    r_init, nsub, E_sedov = 0.1, 4, 1.0
    my_data.get_var("density")[:, :] = 1.0
    my_data.get_var("x-momentum")[:, :] = 0.0
    my_data.get_var("y-momentum")[:, :] = 0.0
    ener = my_data.get_var("energy")
    ener[:, :] = 1.e-5 / (gamma - 1.0)
    # zones near the blast: the pressure is the mean over nsub x nsub sub-samples, summed one after
    # the other in the reference's order (flame.py:57-77) -- vectorised over the zones only
    x2d, y2d = np.asarray(g.x2d), np.asarray(g.y2d)
    si, sj = np.nonzero(np.sqrt((x2d - xctr)**2 + (y2d - yctr)**2) < 2.0 * r_init)
    xl, yl = np.asarray(g.xl), np.asarray(g.yl)
    p_in = (gamma - 1.0) * E_sedov / (math.pi * r_init * r_init)
    pzone = np.zeros(len(si))
    for ii in range(nsub):
        for jj in range(nsub):
            xsub = xl[si] + (g.dx / nsub) * (ii + 0.5)
            ysub = yl[sj] + (g.dy / nsub) * (jj + 0.5)
            dist = np.sqrt((xsub - xctr)**2 + (ysub - yctr)**2)
            pzone = pzone + np.where(dist <= r_init, p_in, 1.e-5)
    ener[si, sj] = (pzone / (nsub * nsub)) / (gamma - 1.0)


def finalize():
    print("\n  The blast is the Sedov problem's: compare the radial profiles of density, velocity and\n"
          "  pressure with the cylindrical Sedov solution; fuel and ash stay at zero.\n")
