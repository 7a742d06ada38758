"""A smooth velocity field for convergence tests: both components are
A + A exp(-50 r^2) around the centre of the domain, A = 0.05 (reference:
pyro/burgers/problems/converge.py).  inputs.converge.32 / 64 / 128 / 256 halve
the fixed time step with the mesh spacing."""
import numpy as np

from ...util import msg

DEFAULT_INPUTS = "inputs.converge.64"
PROBLEM_PARAMS = {}


def init_data(myd, rp):
    if rp.get_param("driver.verbose"):
        msg.bold("initializing the smooth burgers convergence problem...")
    g = myd.grid
    xctr = 0.5 * (g.xmin + g.xmax)
    yctr = 0.5 * (g.ymin + g.ymax)
    A = 0.05
    r2 = (np.asarray(g.x2d) - xctr)**2 + (np.asarray(g.y2d) - yctr)**2
    for name in ("x-velocity", "y-velocity"):
        myd.get_var(name)[:, :] = A + A * np.exp(-50.0 * r2)


def finalize():
    pass
