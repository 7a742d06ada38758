"""advection_fv4.Simulation with the call surface of pyro/advection_fv4/simulation.py:9-76:
advection_rk's driver on cell averages (mesh/fv.py FV2d) with the fourth-order fluxes of
McCorquodale & Colella (pyrohip_advrk_params.scheme = 4)."""
from ..advection_rk.simulation import Simulation as RKSimulation
from ..mesh import fv
from ..mesh import patch


class Simulation(RKSimulation):
    scheme = 4
    # the data of a restart file are averages already: preevolve is not run over them
    restart_skips_preevolve = True

    def __init__(self, solver_name, problem_name, problem_func, rp, *,
                 problem_finalize_func=None, problem_source_func=None,
                 timers=None, data_class=fv.FV2d):
        if data_class is patch.CellCenterData2d:
            data_class = fv.FV2d
        super().__init__(solver_name, problem_name, problem_func, rp,
                         problem_finalize_func=problem_finalize_func,
                         problem_source_func=problem_source_func,
                         timers=timers, data_class=data_class)

    def preevolve(self):
        """the problem set up cell centres: convert them to averages
        (advection_fv4/simulation.py:65-76), on the device"""
        for var in self.cc_data.names:
            self.cc_data.from_centers(var)
