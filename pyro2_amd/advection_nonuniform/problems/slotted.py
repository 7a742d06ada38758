"""Disc of radius 0.15 with a slot cut into it, in a velocity field that turns it rigidly
about the centre of the domain (reference: advection_nonuniform/problems/slotted.py): one
revolution shows how well the scheme keeps the shape."""
import numpy as np

from ...util import msg

DEFAULT_INPUTS = "inputs.slotted"
PROBLEM_PARAMS = {"slotted.omega": 0.5,      # angular velocity
                  "slotted.offset": 0.25}    # the disc's centre above the domain's


def init_data(myd, rp):
    if rp.get_param("driver.verbose"):
        msg.bold("initializing the slotted advection problem...")
    offset = rp.get_param("slotted.offset")
    omega = rp.get_param("slotted.omega")
    g = myd.grid
    xc = 0.5 * (g.xmin + g.xmax)
    yc = 0.5 * (g.ymin + g.ymax) + offset
    R, width = 0.15, 0.05
    dens = myd.get_var("density")
    dens[:, :] = 0.0
    dens[(g.x2d - xc)**2 + (g.y2d - yc)**2 < R**2] = 1.0
    in_x = np.logical_and(g.x2d > (xc - width * 0.5), g.x2d < (xc + width * 0.5))
    in_y = np.logical_and(g.y2d > (yc - R), g.y2d < yc)
    dens[np.logical_and(in_x, in_y)] = 0.0
    # rigid rotation (the reference measures y from the x centre and x from the y centre
    # less the offset: the same point on its square domain)
    u = myd.get_var("x-velocity")
    v = myd.get_var("y-velocity")
    u[:, :] = omega * (g.y2d - xc)
    v[:, :] = -omega * (g.x2d - (yc - offset))
    print("extrema: ", np.amax(u), np.amin(u))


def finalize():
    pass
