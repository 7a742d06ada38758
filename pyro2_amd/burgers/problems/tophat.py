"""A disc of radius 0.1 in the middle of the domain moving with (u, v) = (1, 1)
through fluid at rest: its leading edge steepens into a shock (reference:
pyro/burgers/problems/tophat.py)."""
import numpy as np

from ...util import msg

DEFAULT_INPUTS = "inputs.tophat"
PROBLEM_PARAMS = {}


def init_data(myd, rp):
    if rp.get_param("driver.verbose"):
        msg.bold("initializing the tophat burgers problem...")
    g = myd.grid
    xctr = 0.5 * (g.xmin + g.xmax)
    yctr = 0.5 * (g.ymin + g.ymax)
    R = 0.1
    inside = (np.asarray(g.x2d) - xctr)**2 + (np.asarray(g.y2d) - yctr)**2 < R**2
    for name in ("x-velocity", "y-velocity"):
        myd.get_var(name)[:, :] = np.where(inside, 1.0, 0.0)


def finalize():
    pass
