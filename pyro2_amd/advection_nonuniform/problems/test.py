"""uniform density in a uniform diagonal flow, used by unit tests (reference:
advection_nonuniform/problems/test.py)"""
DEFAULT_INPUTS = None
PROBLEM_PARAMS = {}


def init_data(my_data, rp):
    del rp
    my_data.get_var("density")[:, :] = 1.0
    my_data.get_var("x-velocity")[:, :] = 1.0
    my_data.get_var("y-velocity")[:, :] = 1.0


def finalize():
    pass
