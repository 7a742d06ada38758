"""Solver-independent Simulation base class and grid / BC set-up helpers with
the surface of pyro/simulation_null.py:10-300.  Host side: this is the caller
of the device hot path, its time-step policy (compute_timestep) is part of the
boundary that must be preserved exactly."""
import numpy as np

from .mesh import boundary as bnd
from .mesh import patch
from .util import msg
from .util import profile_pyro as profile


def _param(rp, key, default, what):
    try:
        return rp.get_param(key)
    except KeyError:
        msg.warning(f"{key} not set, defaulting to {what}")
        return default


_warned_replicas = False


def grid_setup(rp, ng=1, spherical_ok=False, decomposable=False):
    """build the Grid2d described by the [mesh] parameters
    (simulation_null.py:10-69).  spherical_ok: the calling solver has the
    geometry terms (only the compressible solver does, as in the reference).
    decomposable: the calling solver steps x-slabs (compressible, advection): with one process
    per GPU (decomp.active_decomposition: a launcher's RANK / WORLD_SIZE, gpu.decompose) the
    grid handed out is THIS rank's slab of the [mesh] grid -- global xmin / xmax / dx, local nx,
    the coordinates of its rows of the whole grid (mesh/patch.py Grid2d(slab=...))"""
    nx = rp.get_param("mesh.nx")
    ny = rp.get_param("mesh.ny")
    xmin = _param(rp, "mesh.xmin", 0.0, "0.0")
    xmax = _param(rp, "mesh.xmax", 1.0, "1.0")
    ymin = _param(rp, "mesh.ymin", 0.0, "0.0")
    ymax = _param(rp, "mesh.ymax", 1.0, "1.0")
    grid_type = _param(rp, "mesh.grid_type", "Cartesian2d", "Cartesian2D")
    if grid_type == "SphericalPolar":
        if not spherical_ok:
            raise ValueError("mesh.grid_type = SphericalPolar is implemented by the "
                             "compressible solver only")
        return patch.SphericalPolar(nx, ny, xmin=xmin, xmax=xmax, ymin=ymin, ymax=ymax, ng=ng)
    if grid_type != "Cartesian2d":
        raise ValueError("Unsupported grid type!")
    from . import decomp
    dec = decomp.active_decomposition(rp)
    if dec is not None and not decomposable:
        global _warned_replicas
        if not _warned_replicas:
            _warned_replicas = True
            msg.warning(f"{dec.nranks} processes: this solver is not domain-decomposed, every "
                        "process runs the whole problem")
        dec = None
    slab = None
    if dec is not None:
        xlb = _param(rp, "mesh.xlboundary", "periodic", "periodic")
        slab = decomp.SlabDecomp(nx, dec.nranks, dec.rank, periodic=(xlb == "periodic"))
    return patch.Cartesian2d(nx, ny, xmin=xmin, xmax=xmax, ymin=ymin, ymax=ymax, ng=ng, slab=slab)


def bc_setup(rp):
    """(bc, bc_xodd, bc_yodd): scalars reflect evenly, the normal velocity
    component oddly (simulation_null.py:72-112)"""
    sides = [_param(rp, "mesh." + k, "periodic", "periodic")
             for k in ("xlboundary", "xrboundary", "ylboundary", "yrboundary")]
    kw = dict(xlb=sides[0], xrb=sides[1], ylb=sides[2], yrb=sides[3])
    return (bnd.BC(**kw), bnd.BC(odd_reflect_dir="x", **kw), bnd.BC(odd_reflect_dir="y", **kw))


class NullSimulation:
    def __init__(self, solver_name, problem_name, problem_func, rp, *,
                 problem_finalize_func=None, problem_source_func=None,
                 timers=None, data_class=patch.CellCenterData2d):
        self.n = 0
        self.dt = -1.e33
        self.dt_old = -1.e33
        self.data_class = data_class
        self.rp = rp
        self.tmax = self._opt("driver.tmax")
        self.max_steps = self._opt("driver.max_steps")
        self.cc_data = None
        self.particles = None
        self.SMALL = 1.e-12
        self.solver_name = solver_name
        self.problem_name = problem_name
        self.problem_func = problem_func
        self.problem_finalize = problem_finalize_func
        self.problem_source = problem_source_func
        self.tc = timers if timers is not None else profile.TimerCollection()
        v = self._opt("driver.verbose")
        self.verbose = 0 if v is None else v
        self.n_num_out = 0
        self.cm = "viridis"

    def _opt(self, key):
        try:
            return self.rp.get_param(key)
        except (AttributeError, KeyError):
            return None

    def _rp_opt(self, key, default):
        """a runtime parameter that a hand-built RuntimeParameters (the reference's
        unit tests) may not carry"""
        v = self._opt(key)
        return default if v is None else v

    def __str__(self):
        return f"pyro Simulation:\n  solver: {self.solver_name}\n  problem: {self.problem_name}\n"

    # ---- tracer particles (pyro/particles) --------------------------------
    def setup_particles(self, bc):
        """particles.do_particles = 1: seed the tracers the way every solver's
        initialize() does (e.g. advection/simulation.py:30-33)"""
        if self.rp.get_param("particles.do_particles") == 1:
            if getattr(self.cc_data, "slab", None) is not None:
                msg.fail("ERROR: tracer particles are not carried by a decomposed run")
            from .particles import particles
            self.particles = particles.Particles(
                self.cc_data, bc, self.rp.get_param("particles.n_particles"),
                self.rp.get_param("particles.particle_generator"))

    def advance_particles(self, u=None, v=None):
        """move the tracers over self.dt with the cell-centred velocity: the
        arrays given (host path), else the velocity in the evolving state --
        on the device where _device_particle_source() finds it there, else
        on the host from the stored x-/y-velocity or the derived "velocity"
        (which downloads the state)"""
        if self.particles is None:
            return
        cc = self.cc_data
        if u is None and v is None:
            src = self._device_particle_source()
            if src is not None:
                # device_state() carries out a pending ghost fill / upload, as the host
                # path's read of the data would; the state itself is only read
                self.particles.update_particles_device(self.dt, cc.device_state(), *src)
                return
            if "x-velocity" in cc.names:
                u, v = cc.get_var_readonly("x-velocity"), cc.get_var_readonly("y-velocity")
            else:
                u, v = cc.get_var_readonly("velocity")
        self.particles.update_particles(self.dt, u, v)

    def _device_particle_source(self):
        """(mode, plane indices) of the tracers' velocity in the state when they can be
        advanced on the device (gpu.device_particles, boundary kinds the kernel knows,
        stored velocities or momenta over density / height), else None"""
        from . import _lib
        ps, names = self.particles, self.cc_data.names
        if self._rp_opt("gpu.device_particles", 1) != 1 or ps.bc is None:
            return None
        if any(b not in _lib.PART_BC_CODE for b in (ps.bc.xlb, ps.bc.xrb, ps.bc.ylb, ps.bc.yrb)):
            return None
        if ps.n_particles > _lib.PARTICLES_MAX:     # (beyond one scanning workgroup: host path)
            return None
        if "x-velocity" in names:
            if "y-velocity" not in names:
                return None
            return "planes", (names.index("x-velocity"), names.index("y-velocity"))
        if "x-momentum" in names and "y-momentum" in names:
            for den in ("density", "height"):
                if den in names:
                    return "ratio", (names.index("x-momentum"), names.index("y-momentum"),
                                     names.index(den))
        return None

    def finished(self):
        return self.cc_data.t >= self.tmax or self.n >= self.max_steps

    def do_output(self):
        dt_out = self.rp.get_param("io.dt_out")
        n_out = self.rp.get_param("io.n_out")
        do_io = self.rp.get_param("io.do_io")
        due = self.cc_data.t >= (self.n_num_out + 1) * dt_out or self.n % n_out == 0
        if due and do_io == 1:
            self.n_num_out += 1
            return True
        return False

    def initialize(self):
        pass

    def method_compute_timestep(self):
        """solver specific CFL step -> self.dt"""

    def compute_timestep(self):
        """driver policy around the solver's CFL step: fixed dt, small first
        step, bounded growth, and landing exactly on tmax
        (simulation_null.py:222-244)"""
        init_tstep_factor = self.rp.get_param("driver.init_tstep_factor")
        max_dt_change = self.rp.get_param("driver.max_dt_change")
        fix_dt = self.rp.get_param("driver.fix_dt")
        if fix_dt > 0.0:
            self.dt = fix_dt
        else:
            self.method_compute_timestep()
            if self.n == 0:
                self.dt = init_tstep_factor * self.dt
            else:
                self.dt = min(max_dt_change * self.dt_old, self.dt)
            self.dt_old = self.dt
        if self.cc_data.t + self.dt > self.tmax:
            self.dt = self.tmax - self.cc_data.t

    def _evolve_by_device_policy(self, nsteps, start, call, refusable=False):
        """evolve_many of the solvers whose dt policy runs in a kernel: up to
        nsteps of fill_BC_all + compute_timestep + evolve without a host round trip per step.
        start() -> device state (and what the solver does first); call(state, policy, cfl,
        nsteps, particles) -> the time steps taken, `particles` being what the device state's
        *_evolve methods take: the tracer set, advanced on the device behind every step
        (DESIGN.md 15.1), or None.  refusable: the library's own rules for device-side
        stepping are stricter than can_evolve_many's -- a refusal before the first step means
        "step singly from now on"."""
        from ._lib import PyroHipError
        from .decomp import DtPolicy
        rp = self.rp
        pol = DtPolicy(self.tmax, rp.get_param("driver.init_tstep_factor"),
                       rp.get_param("driver.max_dt_change"), rp.get_param("driver.fix_dt"))
        pol.t, pol.n = float(self.cc_data.t), int(self.n)
        pol.dt_old = float(getattr(self, "dt_old", -1.e33))
        tm = self.tc.timer("evolve")
        tm.begin()
        st = start()
        bound = None
        if self.particles is not None:
            # (can_evolve_many: only a set the device can advance gets here)
            bound = self.particles.device_binding(st.ctx, *self._device_particle_source())
        try:
            dts = call(st, pol, float(rp.get_param("driver.cfl")), int(nsteps), bound)
        except PyroHipError as e:
            if not refusable or "device-side stepping:" not in str(e) or pol.n != int(self.n):
                raise
            self._device_stepping_refused = True
            dts = []
        finally:
            self.cc_data.device_modified()
            if bound is not None:
                self.particles.device_ran()
            self.cc_data.t, self.n, self.dt_old = pol.t, pol.n, pol.dt_old
        if len(dts):
            self.dt = float(dts[-1])
        tm.end()
        return dts

    def _plan_timesteps(self, nsteps, usable):
        """evolve_many of the solvers whose CFL step is closed-form: the driver's policy gives the
        dt sequence of up to nsteps iterations beforehand -- computed by the very methods the
        single step uses; t and n are left where they were.  usable(dt): the solver's own test."""
        cc = self.cc_data
        t0, n0 = cc.t, self.n
        dts = []
        while len(dts) < nsteps and not self.finished():
            keep = (getattr(self, "dt", None), getattr(self, "dt_old", None))
            self.compute_timestep()
            if not usable(self.dt):
                # no usable step to hand to the device: undo this policy call (t, n were not
                # advanced for it) and let the driver take the step singly, like the reference
                self.dt, self.dt_old = keep
                break
            dts.append(float(self.dt))
            cc.t += self.dt                      # as evolve() does
            self.n += 1
        cc.t, self.n = t0, n0
        return dts

    def preevolve(self):
        pass

    def evolve(self):
        self.cc_data.t += self.dt
        self.n += 1

    def dovis(self):
        pass

    def finalize(self):
        if self.problem_finalize:
            self.problem_finalize()

    def write(self, filename):
        """HDF5 dump in the reference layout (simulation_null.py:270-290);
        this is a device -> host synchronisation point"""
        from .util import h5lite
        cc = self.cc_data
        if getattr(cc, "slab", None) is not None:
            # COLLECTIVE: the slabs are gathered, rank 0 writes the ONE file of the reference's
            # layout (state/<var>/data is the whole nx x ny array, patch.py:750-788)
            if self.particles is not None:
                msg.fail("ERROR: tracer particles are not carried by a decomposed run")
            whole = cc.gather()
            if whole is None:
                return
            keep, self.cc_data = self.cc_data, whole
            try:
                self._write_one(filename)
            finally:
                self.cc_data = keep
            return
        self._write_one(filename)

    def _write_one(self, filename):
        from .util import h5lite
        with h5lite.open_file(filename, "w") as f:
            f.attrs["solver"] = self.solver_name
            f.attrs["problem"] = self.problem_name
            f.attrs["time"] = self.cc_data.t
            f.attrs["nsteps"] = self.n
            # not in the reference's files: lets a restart reproduce the
            # max_dt_change limiter of the next step exactly
            f.attrs["dt"] = self.dt
            f.attrs["dt_old"] = self.dt_old
            try:      # which arithmetic wrote the file (0: bit-faithful, 1: contracted)
                f.attrs["gpu_fast_math"] = int(self.rp.get_param("gpu.fast_math"))
            except (KeyError, RuntimeError, ValueError):
                pass
            self.cc_data.write_data(f)
            if self.particles is not None:
                self.particles.write_particles(f)
            self.rp.write_params(f)
            self.write_extras(f)

    def write_extras(self, f):
        pass

    def read_extras(self, f):
        pass
