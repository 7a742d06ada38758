"""Pin the C oracle (oracle/pyro_oracle.c) against the reference.

The fixtures under tests/golden/ were produced by oracle/gen_golden.py, which
RUNS the reference (pyro2) in the build container, and include the
reference's own regression goldens (pyro/test.py:93,100-101,138-140).
"""
import numpy as np
import pytest

from oracle import orc


# ---------------------------------------------------------------- ghost fill
@pytest.mark.parametrize("ng", [4, 1])
@pytest.mark.parametrize("k", range(5))
def test_fill_ghost(golden, ng, k):
    g = golden("fill_bc")
    a = g[f"in_ng{ng}_{k}"].copy()
    bcs = [str(b) for b in g[f"bc_ng{ng}_{k}"]]
    nx, ny = a.shape[0] - 2 * ng, a.shape[1] - 2 * ng
    orc.fill_ghost(a, nx, ny, ng, bcs)
    assert np.array_equal(a, g[f"out_ng{ng}_{k}"])


# ----------------------------------------------------------------- advection
def test_adv_stages(golden):
    g = golden("adv_stages")
    n = int(g["ncases"])
    assert n >= 10
    for k in range(n):
        nx, ny, ng, dx, dy, u, v, dt, lim = g[f"s{k}_meta"]
        nx, ny, ng, lim = int(nx), int(ny), int(ng), int(lim)
        a = g[f"s{k}_a0"].copy()
        assert np.array_equal(orc.limit(a, nx, ny, ng, 1, lim), g[f"s{k}_ldx"])
        assert np.array_equal(orc.limit(a, nx, ny, ng, 2, lim), g[f"s{k}_ldy"])
        st = orc.adv_step(a, nx, ny, ng, dx, dy, u, v, dt, lim, stages=True)
        for nm in ("ldx", "ldy", "ax", "ay", "Fx", "Fy"):
            assert np.array_equal(st[nm], g[f"s{k}_{nm}"]), (k, nm)
        assert np.array_equal(a, g[f"s{k}_a1"]), k


def _run_adv(ic, dts, nx, ng=4, u=1.0, v=1.0, limiter=2):
    a = ic.copy()
    dx = 1.0 / nx
    for dt in dts:
        orc.fill_ghost(a, nx, nx, ng, ("periodic",) * 4)
        orc.adv_step(a, nx, nx, ng, dx, dx, u, v, dt, limiter)
    return a


def test_adv_reference_regression_smooth_0040(golden):
    """pyro/test.py:93 : advection smooth vs smooth_0040.h5, rtol 1e-12"""
    g = golden("adv_smooth_0040")
    a = _run_adv(g["ic"], g["dts"], 32)
    assert np.array_equal(a[4:-4, 4:-4], g["run"])          # reference run here
    np.testing.assert_allclose(a[4:-4, 4:-4], g["gold"], rtol=1e-12, atol=0)


def test_adv_dt_and_64_known_answer(golden):
    """64^2 to tmax: 81 steps, L2 error 0.00327229868007
    (pyro/advection/tests/advection_convergence.txt:8)"""
    g = golden("adv_smooth_64")
    dts = g["dts"]
    assert len(dts) == 81
    assert orc.adv_dt(1 / 64, 1 / 64, 1.0, 1.0, 0.8) == dts[0]
    a = _run_adv(g["ic"], dts, 64)
    assert np.array_equal(a[4:-4, 4:-4], g["final"][4:-4, 4:-4])
    err = a[4:-4, 4:-4] - g["ic"][4:-4, 4:-4]
    l2 = np.sqrt((1 / 64) ** 2 * np.sum(err ** 2))
    assert abs(l2 - 0.00327229868007) < 1e-13


# ---------------------------------------------------------------- multigrid
_MGBC = {"dirichlet": "dirichlet", "neumann": "neumann", "periodic": "periodic"}


def _mk_mg(g, k):
    nx, alpha, beta, ns, nb, inhom = g[f"m{k}_meta"]
    bcs = [str(b) for b in g[f"m{k}_bc"]]
    m = orc.MG(int(nx), bcs=bcs, alpha=alpha, beta=beta, nsmooth=int(ns),
               nsmooth_bottom=int(nb))
    if int(inhom):
        for s in range(4):
            m.set_bcval(s, g[f"m{k}_bcvals"][s])
    return m


def test_mg_ops(golden):
    g = golden("mg_ops")
    n = int(g["ncases"])
    assert n >= 12
    for k in range(n):
        m = _mk_mg(g, k)
        L = m.nlevels - 1
        m.arr(L, 0)[:, :] = g[f"m{k}_v0"]
        m.init_rhs(g[f"m{k}_f0"])
        m.smooth(L, 2)
        assert np.array_equal(m.arr(L, 0), g[f"m{k}_v_smooth"]), k
        m.residual(L)
        assert np.array_equal(m.arr(L, 2), g[f"m{k}_r"]), k
        np.testing.assert_allclose(m.norm(L, 2), g[f"m{k}_rnorm"], rtol=1e-14)
        m.restrict(L)
        assert np.array_equal(m.arr(L - 1, 1)[1:-1, 1:-1],
                              g[f"m{k}_restrict"][1:-1, 1:-1]), k
        # prolong: v_fine := 0; v_fine += prolong(cv)
        m.arr(L - 1, 0)[:, :] = g[f"m{k}_cv"]
        m.arr(L, 0)[:, :] = 0.0
        m.prolong_add(L)
        assert np.array_equal(m.arr(L, 0)[1:-1, 1:-1],
                              g[f"m{k}_prolong"][1:-1, 1:-1]), k

        m = _mk_mg(g, k)
        m.arr(L, 0)[:, :] = g[f"m{k}_v0"]
        m.init_rhs(g[f"m{k}_f1"])
        m.vcycle()
        assert np.array_equal(m.arr(L, 0), g[f"m{k}_v_vcycle"]), k
        m.solve(rtol=1e-10, max_cycles=6)
        info = g[f"m{k}_solve_info"]
        assert m.num_cycles == int(info[0])
        assert np.array_equal(m.arr(L, 0), g[f"m{k}_v_solve"]), k
        np.testing.assert_allclose(m.residual_error, info[1], rtol=1e-10)
        np.testing.assert_allclose(m.source_norm, info[3], rtol=1e-13)


def test_mg_reference_regression_poisson_dirichlet(golden):
    """pyro/test.py:138-140: mg_test_simple 256^2 vs mg_poisson_dirichlet.h5;
    7 V-cycles, L2 error 1.60408e-06 (multigrid/tests/mg_convergence.txt:7)"""
    g = golden("mg_poisson_dirichlet_256")
    m = orc.MG(256)
    L = m.nlevels - 1
    m.init_rhs(g["rhs"])
    m.solve(rtol=1e-11)
    assert m.num_cycles == int(g["ncycles"]) == 7
    assert np.array_equal(m.arr(L, 0)[1:-1, 1:-1], g["gold"])
    x = (np.arange(258) - 0.5) / 256
    X, Y = np.meshgrid(x, x, indexing="ij")
    true = (X ** 2 - X ** 4) * (Y ** 4 - Y ** 2)
    e = (m.arr(L, 0) - true)[1:-1, 1:-1]
    l2 = np.sqrt(np.sum(e ** 2) / 256 ** 2)
    assert abs(l2 - 1.60408e-06) < 1e-11


# -------------------------------------------------------------- compressible
from helpers import meta_to_params, oracle_comp_run  # noqa: E402
from conftest import max_rel_err  # noqa: E402

_STAGES = ["q", "xi", "ldx", "ldy", "Uxl0", "Uxr0", "Uyl0", "Uyr0", "FxT",
           "FyT", "Uxl", "Uxr", "Uyl", "Uyr", "Fx0", "Fy0", "avx", "avy",
           "Fx", "Fy"]


@pytest.mark.parametrize("k", range(8))
def test_comp_stage_dumps(golden, k):
    """every intermediate array of one step, ghost cells included, against
    arrays dumped from the reference's own functions"""
    g = golden("comp_stages")
    bcs = [str(b) for b in g[f"c{k}_bc"]]
    P, cfl = meta_to_params(g[f"c{k}_meta"], bcs)
    U = g[f"c{k}_U0"].copy()
    dtm = orc.comp_dt(U, P.nx, P.ny, P.ng, P.dx, P.dy, P.gamma, cfl)
    assert dtm == float(g[f"c{k}_dt_method"])
    rc, st = orc.comp_step(U, P, float(g[f"c{k}_dt"]), stages=True)
    assert rc == 0
    worst = 0.0
    for nm in _STAGES:
        e = max_rel_err(st[nm], g[f"c{k}_{nm}"])
        worst = max(worst, e)
        assert e == 0.0, (k, nm, e)   # bit-identical to the reference
    e = max_rel_err(U, g[f"c{k}_U1"])
    assert e == 0.0, (k, "U1", e)


def test_comp_sedov_64_fingerprint(golden):
    """sedov 64^2, 20 steps"""
    g = golden("comp_sedov_64_020")
    bcs = [str(b) for b in g["bc"]]
    U, dts, t = oracle_comp_run(g["ic"], g["meta"], bcs, tmax=0.1, max_steps=20)
    np.testing.assert_allclose(dts, g["dts"], rtol=1e-13, atol=0)
    assert abs(t - 0.009286102192696327) < 1e-15
    assert max_rel_err(U[4:-4, 4:-4], g["final"][4:-4, 4:-4]) < 1e-12
    assert abs(U[4:-4, 4:-4, 1].sum() - 4774.750655256859) < 1e-8


def test_comp_reference_regression_sod_x(golden):
    """pyro/test.py:101: compressible sod inputs.sod.x vs sod_x_0076.h5
    (128x10, limiter 1, reflecting y walls), rtol 1e-12"""
    g = golden("comp_sod_x_0076")
    bcs = [str(b) for b in g["bc"]]
    U, dts, t = oracle_comp_run(g["ic"], g["meta"], bcs, tmax=float(g["tmax"]),
                                max_steps=200)
    assert len(dts) == 76
    np.testing.assert_allclose(dts, g["dts"], rtol=1e-12, atol=0)
    for n in range(4):
        assert max_rel_err(U[4:-4, 4:-4, n], g["gold"][..., n]) < 1e-12 or \
            np.abs(g["gold"][..., n]).max() == 0.0


def test_comp_reference_regression_quad(golden):
    """pyro/test.py:100: compressible quad inputs.quad vs
    quad_unsplit_0606.h5 (256^2, 606 steps, HLLC, limiter 2).  The reference
    itself cannot be re-run at this size here (interpreted njit loops), so
    this is the oracle reproducing the reference's STORED golden from the
    reference's IC."""
    g = golden("comp_quad_0606")
    bcs = [str(b) for b in g["bc"]]
    U, dts, t = oracle_comp_run(g["ic"], g["meta"], bcs, tmax=float(g["tmax"]),
                                max_steps=1000)
    assert len(dts) == int(g["nsteps"]) == 606
    assert abs(t - float(g["t"])) < 1e-14
    for n in range(4):
        e = max_rel_err(U[4:-4, 4:-4, n], g["gold"][..., n])
        assert e < 1e-12, (n, e)   # measured 1.0e-13 (golden made with real numba)


def test_comp_reference_regression_rt(golden):
    """pyro/test.py:102: compressible rt inputs.rt vs rt_0945.h5 (64x192, 945
    steps; gravity + hse boundaries): the oracle reproducing the reference's
    STORED golden from the reference's IC.  RT growth amplifies round-off, so
    the momenta are compared relative to the largest momentum."""
    g = golden("comp_rt_0945")
    bcs = [str(b) for b in g["bc"]]
    f0, mx = g["drv"]
    U, dts, t = oracle_comp_run(g["ic"], g["meta"], bcs, float(g["tmax"]), 10000, f0, mx)
    assert len(dts) == int(g["nsteps"]) == 945
    assert abs(t - float(g["t"])) < 1e-13
    gold = g["gold"]
    scale = np.abs(gold).max(axis=(0, 1))
    err = np.abs(U[4:-4, 4:-4] - gold).max(axis=(0, 1)) / scale
    assert err.max() < 1e-11, err


def test_mg_variable_coefficient(golden):
    """variable_coeff_MG.VarCoeffCCMG2d: edge coefficients on three levels,
    smoother, residual and a 5-cycle solve against the reference"""
    g = golden("mg_vc")
    for k in range(int(g["ncases"])):
        nx = int(g[f"v{k}_nx"])
        m = orc.VCMG(nx, g[f"v{k}_c"], bcs=[str(b) for b in g[f"v{k}_bc"]],
                     coeffs_bcs=[str(b) for b in g[f"v{k}_cbc"]], nsmooth=4, nsmooth_bottom=9)
        L = m.nlevels - 1
        for lev in (L, L - 1, 0):
            n = 2 ** (lev + 1)
            assert np.array_equal(m.coef(lev, 0), g[f"v{k}_c_l{lev}"]), (k, lev)
            # x edges valid for i in [1, n+1], j interior (and vice versa)
            assert np.array_equal(m.coef(lev, 1)[1:n + 2, 1:n + 1], g[f"v{k}_ex_l{lev}"][1:n + 2, 1:n + 1])
            assert np.array_equal(m.coef(lev, 2)[1:n + 1, 1:n + 2], g[f"v{k}_ey_l{lev}"][1:n + 1, 1:n + 2])
        m.arr(L, 0)[:, :] = g[f"v{k}_v0"]
        m.init_rhs(g[f"v{k}_f0"])
        m.smooth(L, 3)
        assert np.array_equal(m.arr(L, 0), g[f"v{k}_v_smooth"]), k
        m.residual(L)
        assert np.array_equal(m.arr(L, 2)[1:-1, 1:-1], g[f"v{k}_r"][1:-1, 1:-1]), k
        m.arr(L, 0)[:, :] = g[f"v{k}_v0"]
        m.solve(rtol=1e-10, max_cycles=5)
        info = g[f"v{k}_info"]
        assert m.num_cycles == int(info[0])
        assert np.array_equal(m.arr(L, 0), g[f"v{k}_v_solve"]), k


def test_mg_general(golden):
    """general_MG.GeneralMG2d: coefficient hierarchy (alpha, gamma restricted,
    beta on edges), smoother, residual and a 5-cycle solve against the reference"""
    g = golden("mg_general")
    for k in range(int(g["ncases"])):
        pre = f"g{k}_"
        nx = int(g[pre + "nx"])
        m = orc.GenMG(nx, g[pre + "alpha"], g[pre + "beta"], g[pre + "gamma_x"], g[pre + "gamma_y"],
                      bcs=[str(b) for b in g[pre + "bc"]],
                      coeffs_bcs=[str(b) for b in g[pre + "cbc"]], nsmooth=4, nsmooth_bottom=9)
        L = m.nlevels - 1
        for lev in (L, L - 1, 0):
            n = 2 ** (lev + 1)
            for which, nm in ((3, "alpha"), (4, "gamma_x"), (5, "gamma_y")):
                assert np.array_equal(m.coef(lev, which), g[pre + f"{nm}_l{lev}"]), (k, lev, nm)
            assert np.array_equal(m.coef(lev, 1)[1:n + 2, 1:n + 1], g[pre + f"ex_l{lev}"][1:n + 2, 1:n + 1])
            assert np.array_equal(m.coef(lev, 2)[1:n + 1, 1:n + 2], g[pre + f"ey_l{lev}"][1:n + 1, 1:n + 2])
        m.arr(L, 0)[:, :] = g[pre + "v0"]
        m.init_rhs(g[pre + "f0"])
        m.smooth(L, 3)
        assert np.array_equal(m.arr(L, 0), g[pre + "v_smooth"]), k
        m.residual(L)
        assert np.array_equal(m.arr(L, 2)[1:-1, 1:-1], g[pre + "r"][1:-1, 1:-1]), k
        m.arr(L, 0)[:, :] = g[pre + "v0"]
        m.solve(rtol=1e-10, max_cycles=5)
        assert m.num_cycles == int(g[pre + "info"][0])
        assert np.array_equal(m.arr(L, 0), g[pre + "v_solve"]), k


@pytest.mark.parametrize("k", range(6))
def test_comp_cgf_and_sponge(golden, k):
    """riemann_cgf (riemann.py:8-310) incl. the solid-wall
    rule, and the sponge (simulation.py:164-184,427-441), against dumps of
    the reference's own functions"""
    g = golden("comp_stages_f2")
    bcs = [str(b) for b in g[f"c{k}_bc"]]
    sp = g[f"c{k}_sponge"]
    P, cfl = meta_to_params(g[f"c{k}_meta"], bcs, riemann=str(g[f"c{k}_riemann"]),
                            sponge=tuple(sp[1:]) if sp[0] else None)
    U = g[f"c{k}_U0"].copy()
    rc, st = orc.comp_step(U, P, float(g[f"c{k}_dt"]), stages=True)
    assert rc == 0
    for nm in ("FxT", "FyT", "Fx0", "Fy0", "Fx", "Fy"):
        assert max_rel_err(st[nm], g[f"c{k}_{nm}"]) == 0.0, (k, nm)
    # the sponge evaluates cos(): libm vs NumPy may differ in the last bit
    tol = 1e-15 if sp[0] else 0.0
    assert max_rel_err(U, g[f"c{k}_U1"]) <= tol, k


# ---------------------------------------------------------------------------
# row f2: gravity + the hse / ambient user boundaries (compressible/BC.py)
# ---------------------------------------------------------------------------
HSE_RIEMANN = {1: "CGF"}


@pytest.mark.parametrize("k", range(4))
def test_oracle_hse_runs(golden, k):
    from helpers import meta_to_params, oracle_comp_run
    g = golden("comp_hse")
    pre = f"c{k}_"
    meta, bcs = g[pre + "meta"], [str(b) for b in g[pre + "bc"]]
    amb = tuple(g[pre + "ambient"])
    f0, mx = g[pre + "drv"]
    dts_ref = g[pre + "dts"]
    over = {"riemann": HSE_RIEMANN.get(k, "HLLC")}
    if k == 1:
        # numba turns the scalar `x**2` of riemann_cgf into x*x (the oracle's
        # default); the goldens come from the interpreted shim, where it is
        # libm pow(x, 2.0).  One face of this run is a case where the two
        # differ by an ulp: default arithmetic agrees to round-off ...
        U, dts, _ = oracle_comp_run(g[pre + "ic"], meta, bcs, 1.e30, len(dts_ref), f0, mx,
                                    ambient=amb, **over)
        assert np.array_equal(dts, dts_ref)
        assert np.allclose(U, g[pre + "final"], rtol=1e-13, atol=1e-12)
        # ... and the shim's arithmetic reproduces them bit for bit
        orc.set_scalar_pow(1)
    try:
        U, dts, _ = oracle_comp_run(g[pre + "ic"], meta, bcs, 1.e30, len(dts_ref), f0, mx,
                                    ambient=amb, **over)
    finally:
        orc.set_scalar_pow(0)
    assert np.array_equal(dts, dts_ref)
    fin = g[pre + "final"]
    ng = int(meta[2])
    assert np.array_equal(U[ng:-ng, ng:-ng], fin[ng:-ng, ng:-ng])
    # ghost cells are whatever the last fill left, also in the reference
    assert np.array_equal(U, fin, equal_nan=True)
    # one more fill + stage dump
    P, _ = meta_to_params(meta, bcs, **over)
    orc.comp_fill_bc(U, P.nx, P.ny, P.ng, bcs, P.gamma, P.grav, P.dy, amb)
    assert np.array_equal(U, g[pre + "filled"])
    rc, st = orc.comp_step(U, P, float(g[pre + "dt"]), stages=True)
    assert rc == 0
    for nm in ("FxT", "FyT", "Fx", "Fy"):
        assert np.array_equal(st[nm], g[pre + nm]), nm
    assert np.array_equal(U[ng:-ng, ng:-ng], g[pre + "U1"][ng:-ng, ng:-ng])


def test_oracle_floored_ghost_image_under_gravity(golden):
    """small_dens + gravity beside a periodic side (oracle/gen_ctu_floor_golden.py: one step of the
    reference from a state with floored cells in the first and the last column, 8 x 57): the source of a
    ghost cell is the FILL of the interior's source (unsplit_fluxes.py:295-306), i.e. that of the floored
    cell it mirrors, while the ghost state keeps the unfloored density (simulation.py:452-456).  The
    oracle's fill, dt and step against the reference's, bit for bit; the cells whose stencil reaches such
    a ghost cell are among those the floor moves"""
    g = golden("comp_floor_grav")
    nx, ny, ng = (int(v) for v in g["grid"])
    gamma, lim, flat, grav, sd, cfl = (float(v) for v in g["params"])
    bcs = [str(b) for b in g["bc"]]
    dx, dy = (float(v) for v in g["dxdy"])
    U = g["U0"].copy()
    orc.comp_fill_bc(U, nx, ny, ng, bcs, gamma, grav, dy)
    assert np.array_equal(U, g["U0"])
    assert orc.comp_dt(U, nx, ny, ng, dx, dy, gamma, cfl) == float(g["dt"])
    I = (slice(ng, -ng), slice(ng, -ng))
    floored = np.argwhere(U[I][..., 0] < sd)
    assert [1, 0] in floored.tolist() and [nx - 2, ny - 1] in floored.tolist()
    assert U[ng + 1, ng + ny, 0] < sd and U[ng + nx - 2, ng - 1, 0] < sd       # their unfloored ghost images
    P = orc.comp_params(nx, ny, ng, dx, dy, gamma=gamma, limiter=int(lim), use_flattening=int(flat), grav=grav,
                        small_dens=sd, bcs=tuple(bcs))
    assert orc.comp_step(U, P, float(g["dt"]))[0] == 0
    assert np.array_equal(U[I], g["U1"][I])
    assert np.array_equal(U[:, :ng], g["U0"][:, :ng])                   # the ghost cells stay as filled
    # (the source of the ghost images decides something: with the floor a hair lower the cells beside them move)
    V = g["U0"].copy()
    P.small_dens = 0.9 * sd
    assert orc.comp_step(V, P, float(g["dt"]))[0] == 0
    assert all(not np.array_equal(V[I][c], g["U1"][I][c]) for c in ((0, ny - 1), (nx - 1, 0)))


# ---------------------------------------------------------------------------
# rows f1 / f4: burgers and the incompressible projection solver
# ---------------------------------------------------------------------------
def _bg_run(ic, meta, bcs, nsteps, tmax=0.1):
    nx, ny, ng, dx, dy, lim, cfl = meta
    nx, ny, ng, lim = int(nx), int(ny), int(ng), int(lim)
    u, v = ic[0].copy(), ic[1].copy()
    t, dts = 0.0, []
    for _ in range(nsteps):
        orc.fill_ghost(u, nx, ny, ng, bcs)
        orc.fill_ghost(v, nx, ny, ng, bcs)
        dt = orc.bg_dt(u, v, nx, ny, ng, dx, dy, cfl)   # inputs.test: no start-up limiter
        if t + dt > tmax:
            dt = tmax - t
        orc.bg_step(u, v, nx, ny, ng, dx, dy, dt, lim)
        t += dt
        dts.append(dt)
    return u, v, np.array(dts)


@pytest.mark.parametrize("k", range(2))
def test_oracle_burgers(golden, k):
    g = golden("incomp")
    pre = f"b{k}_"
    meta, bcs = g[pre + "meta"], [str(b) for b in g[pre + "bc"]]
    dts_ref = g[pre + "dts"]
    u, v, dts = _bg_run(g[pre + "ic"], meta, bcs, len(dts_ref))
    assert np.array_equal(dts, dts_ref)
    ng = int(meta[2])
    fin = g[pre + "final"]
    assert np.array_equal(u[ng:-ng, ng:-ng], fin[0][ng:-ng, ng:-ng])
    assert np.array_equal(v[ng:-ng, ng:-ng], fin[1][ng:-ng, ng:-ng])
    # edge states of one more step: everything the update can reach (B1)
    U0 = g[pre + "U0"]
    nx, ny = int(meta[0]), int(meta[1])
    E = orc.bg_edge_states(U0[0].copy(), U0[1].copy(), None, None, nx, ny, ng, meta[3], meta[4],
                           float(g[pre + "dt"]), int(meta[5]))
    assert np.array_equal(E, g[pre + "E"])


def _inc_bcs():
    return dict(bc_u=("periodic",) * 4, bc_v=("periodic",) * 4, bc_phi=("periodic",) * 4)


@pytest.mark.parametrize("k", range(2))
def test_oracle_incompressible(golden, k):
    """preevolve, a short run and the MAC velocities of one more step against
    the reference (bit-identical up to the solves: the oracle's norms are
    plain sums, NumPy's are pairwise -- see orc_mg_norm -- so the V-cycle
    count at the rtol threshold could differ; it does not in these cases)"""
    from helpers import DtPolicy
    g = golden("incomp")
    pre = f"i{k}_"
    nx, ng, lim, proj, cfl, f0, mx = g[pre + "meta"]
    nx, ng, lim, proj = int(nx), int(ng), int(lim), int(proj)
    dx = 1.0 / nx
    D = np.ascontiguousarray(g[pre + "ic"])
    orc.incomp_preevolve(D, nx, ng, cfl, lim, proj, **_inc_bcs())
    assert np.abs(D - g[pre + "after_pre"]).max() < 1e-13
    pol = DtPolicy(1.e30, f0, mx)
    dts = []
    for _ in g[pre + "dts"]:
        for n in range(6):     # Pyro.single_step: fill_BC_all, also phi and grad p
            orc.fill_ghost(D[n], nx, nx, ng, ("periodic",) * 4)
        dt = pol(orc.bg_dt(D[0], D[1], nx, nx, ng, dx, dx, cfl))
        orc.incomp_step(D, nx, ng, dt, lim, proj, **_inc_bcs())
        pol.advance(dt)
        dts.append(dt)
    assert np.abs(np.array(dts) / g[pre + "dts"] - 1).max() < 1e-12
    fin = g[pre + "final"]
    I = (slice(None), slice(ng, -ng), slice(ng, -ng))
    assert np.abs(D[I] - fin[I]).max() < 1e-11
    # one step from the reference's state, with its dt
    D = np.ascontiguousarray(g[pre + "U0"])
    st = orc.incomp_step(D, nx, ng, float(g[pre + "dt"]), lim, proj, stages=True, **_inc_bcs())
    F = (slice(ng, ng + nx + 1), slice(ng, ng + nx))
    assert np.abs(st["umac"][F] - g[pre + "umac"][F]).max() < 1e-12
    F = (slice(ng, ng + nx), slice(ng, ng + nx + 1))
    assert np.abs(st["vmac"][F] - g[pre + "vmac"][F]).max() < 1e-12
    assert np.abs(D[I] - g[pre + "U1"][I]).max() < 1e-11


def _oracle_shear_run(g):
    from helpers import DtPolicy
    nx, ng, lim, proj, cfl, f0, mx = g["meta"]
    nx, ng, lim, proj = int(nx), int(ng), int(lim), int(proj)
    q = nx + 2 * ng
    D = np.zeros((6, q, q))
    D[:2] = g["ic"]
    orc.incomp_preevolve(D, nx, ng, cfl, lim, proj, **_inc_bcs())
    pol = DtPolicy(float(g["tmax"]), f0, mx)
    while pol.t < float(g["tmax"]) and pol.n < 2000:
        for n in range(6):
            orc.fill_ghost(D[n], nx, nx, ng, ("periodic",) * 4)
        dt = pol(orc.bg_dt(D[0], D[1], nx, nx, ng, 1.0 / nx, 1.0 / nx, cfl))
        orc.incomp_step(D, nx, ng, dt, lim, proj, **_inc_bcs())
        pol.advance(dt)
    return D, pol


def test_incompressible_reference_regression_shear(golden):
    """pyro/test.py:110: incompressible shear inputs.shear vs
    shear_128_0216.h5 (128^2, 216 steps, two MG solves per step): the oracle
    from the reference's IC against the reference's stored golden"""
    g = golden("incomp_shear_128_0216")
    D, pol = _oracle_shear_run(g)
    assert pol.n == int(g["nsteps"]) == 216
    assert abs(pol.t - float(g["t"])) < 1e-13
    ng = int(g["meta"][1])
    I = (slice(ng, -ng), slice(ng, -ng))
    assert np.abs(D[0][I] - g["gold"][0]).max() < 1e-10
    assert np.abs(D[1][I] - g["gold"][1]).max() < 1e-10
    assert np.abs(D[4][I] - g["gold_gp"][0]).max() < 1e-9


# ---------------------------------------------------------------------------
# row f4: compressible_rk (method of lines, RK2 / TVD2 / TVD3 / RK4)
# ---------------------------------------------------------------------------
def _rk_case(g, k):
    pre = f"c{k}_"
    sp = g[pre + "sponge"]
    over = {"riemann": str(g[pre + "riemann"])}
    if sp[0]:
        over["sponge"] = tuple(sp[1:])
    return pre, g[pre + "meta"], [str(b) for b in g[pre + "bc"]], str(g[pre + "method"]), over


@pytest.mark.parametrize("k", range(4))
def test_oracle_compressible_rk(golden, k):
    from helpers import meta_to_params, oracle_rk_run
    g = golden("comp_rk")
    pre, meta, bcs, method, over = _rk_case(g, k)
    ng = int(meta[2])
    I = (slice(ng, -ng), slice(ng, -ng))
    # right-hand side of a reference state
    P, _ = meta_to_params(meta, bcs, **over)
    U0 = g[pre + "U0"].copy()
    rc, kk = orc.comp_rk_rhs(U0, P)
    assert rc == 0
    if str(g[pre + "riemann"]) == "CGF":      # shim: scalar x**2 is libm pow there
        orc.set_scalar_pow(1)
        try:
            rc, kk = orc.comp_rk_rhs(g[pre + "U0"].copy(), P)
        finally:
            orc.set_scalar_pow(0)
    assert np.array_equal(kk[I], g[pre + "k"][I])
    # whole run
    f0, mx = g[pre + "drv"]
    dts_ref = g[pre + "dts"]
    U, dts = oracle_rk_run(g[pre + "ic"], meta, bcs, len(dts_ref), method, f0, mx, **over)
    scale = np.maximum(np.abs(g[pre + "final"][I]).max(axis=(0, 1)), 1e-3)
    assert np.abs(dts / dts_ref - 1).max() < 1e-13
    assert (np.abs(U[I] - g[pre + "final"][I]) / scale).max() < 1e-12


# ---------------------------------------------------------------------------
# row f4: shallow water (pyro/swe), Roe and HLLC
# ---------------------------------------------------------------------------
def _swe_params(g, pre):
    nx, ny, ng, dx, dy, grav, lim, cfl = g[pre + "meta"]
    return orc.swe_params(nx, ny, ng, dx, dy, grav, lim, str(g[pre + "riemann"])), cfl


def swe_fill(U, P, bcs):
    from oracle.orc import comp_var_bcs
    vb = comp_var_bcs(bcs)      # rows for (even, even, x-odd, y-odd)
    rows = [vb[0], vb[2], vb[3], vb[0]]     # height, x-momentum, y-momentum, fuel
    for n in range(4):
        orc.fill_ghost(U, P.nx, P.ny, P.ng, rows[n], n=n)


def oracle_swe_run(ic, P, cfl, bcs, nsteps, tmax=1.e30, f0=0.01, mx=2.0):
    from helpers import DtPolicy
    U = np.ascontiguousarray(ic, dtype=np.float64).copy()
    pol = DtPolicy(tmax, f0, mx)
    dts = []
    while pol.n < nsteps and pol.t < tmax:
        swe_fill(U, P, bcs)
        dt = pol(orc.swe_dt(U, P, cfl))
        orc.swe_step(U, P, dt)
        pol.advance(dt)
        dts.append(dt)
    return U, np.array(dts), pol


@pytest.mark.parametrize("k", range(5))
def test_oracle_swe(golden, k):
    """the interpreted shim evaluates the scalar x**2 of consFlux / riemann_roe
    with libm pow (numba: x*x): goldens are pinned bit for bit in that mode and
    to round-off in the default one"""
    g = golden("swe")
    pre = f"c{k}_"
    P, cfl = _swe_params(g, pre)
    bcs = [str(b) for b in g[pre + "bc"]]
    ng = P.ng
    I = (slice(ng, -ng), slice(ng, -ng))
    orc.set_scalar_pow(1)
    try:
        U = g[pre + "U0"].copy()
        st = orc.swe_step(U, P, float(g[pre + "dt"]), stages=True)
        for nm in ("Uxl0", "Uxr0", "Uyl0", "Uyr0", "FxT", "FyT", "Fx", "Fy"):
            assert np.array_equal(st[nm], g[pre + nm]), nm
        assert np.array_equal(U[I], g[pre + "U1"][I])
        f0, mx = g[pre + "drv"]
        U, dts, _ = oracle_swe_run(g[pre + "ic"], P, cfl, bcs, len(g[pre + "dts"]), f0=f0, mx=mx)
        assert np.array_equal(dts, g[pre + "dts"])
        assert np.array_equal(U[I], g[pre + "final"][I])
    finally:
        orc.set_scalar_pow(0)
    U, dts, _ = oracle_swe_run(g[pre + "ic"], P, cfl, bcs, len(g[pre + "dts"]), f0=f0, mx=mx)
    assert np.abs(U[I] - g[pre + "final"][I]).max() < 1e-13


def test_oracle_swe_edge(golden):
    """one HLLC step without limiting on blocks with height ratios up to 16 (gen_golden.py:
    gen_swe_edge): face states of negative height.  riemann_hllc's max(smallc, sqrt(g h)) is
    Python's max -- smallc for the NaN root -- and its NaN shock speeds fail every comparison;
    the oracle follows it bit for bit (libm-pow mode, as test_oracle_swe), stages and new state"""
    g = golden("swe_edge")
    P, _ = _swe_params(g, "")
    ng = P.ng
    I = (slice(ng, -ng), slice(ng, -ng))
    assert (g["Uxl0"][ng:-ng + 1, ng:-ng, 0] < 0).any() and (g["Uyr0"][ng:-ng, ng:-ng + 1, 0] < 0).any()
    assert np.isfinite(g["U1"]).all()
    orc.set_scalar_pow(1)
    try:
        U = g["U0"].copy()
        st, counts = orc.swe_step(U, P, float(g["dt"]), stages=True, counts=True)
        assert float(g["dt"]) == orc.swe_dt(g["U0"], P, float(g["meta"][7]))
        for nm in ("Uxl0", "Uxr0", "Uyl0", "Uyr0", "FxT", "FyT", "Fx", "Fy"):
            assert np.array_equal(st[nm], g[nm]), nm
        assert np.array_equal(U[I], g["U1"][I])
        assert min(c["h_l_nonpos"] + c["h_r_nonpos"] for c in counts) > 0
    finally:
        orc.set_scalar_pow(0)
    U = g["U0"].copy()
    orc.swe_step(U, P, float(g["dt"]))
    assert np.abs(U[I] - g["U1"][I]).max() < 1e-13


def test_oracle_swe_dt_hands_on_nan(golden):
    """compute_timestep is cfl * min(xtmp.min(), ytmp.min()) (swe/simulation.py:167-171):
    ndarray.min() hands a NaN on, Python's min(a, b) keeps a unless b < a.  So a NaN cell
    whose x quotient is NaN gives NaN, and one where only the y quotient is NaN (the second
    argument) leaves the x minimum"""
    g = golden("swe_edge")
    P, cfl = _swe_params(g, "")
    U = g["U0"].copy()
    good = orc.swe_dt(U, P, cfl)
    assert np.isfinite(good)

    def numpy_dt(U):
        with np.errstate(invalid="ignore", divide="ignore"):
            h, u, v = U[..., 0], U[..., 1] / U[..., 0], U[..., 2] / U[..., 0]
            cs = np.sqrt(P.g * h)
            return cfl * float(min((P.dx / (abs(u) + cs)).min(), (P.dy / (abs(v) + cs)).min()))
    Un = U.copy()
    Un[5, 7, 0] = -1.0                    # sqrt(g h) is NaN: both quotients
    assert np.isnan(numpy_dt(Un)) and np.isnan(orc.swe_dt(Un, P, cfl))
    Uy = U.copy()
    Uy[5, 7, 2] = np.nan                  # only v: Python's min keeps the x minimum
    want = numpy_dt(Uy)
    assert np.isfinite(want) and orc.swe_dt(Uy, P, cfl) == want


def test_swe_reference_regression_dam(golden):
    """pyro/test.py:113: swe dam inputs.dam.x vs dam_x_0081.h5 (128x10, 81
    steps, Roe): oracle from the reference's IC against the stored golden"""
    g = golden("swe_dam_x_0081")
    P, cfl = _swe_params(g, "")
    bcs = [str(b) for b in g["bc"]]
    U, dts, pol = oracle_swe_run(g["ic"], P, cfl, bcs, 10000, tmax=float(g["tmax"]))
    assert pol.n == 81
    ng = P.ng
    assert np.abs(U[ng:-ng, ng:-ng] - g["gold"]).max() < 1e-12


def test_survey_fingerprints(golden):
    """the fingerprints SURVEY.md 8(c) lists for a fresh reference set-up are the
    ones of the runs behind the fixtures (conda py3.9 / NumPy 1.26)"""
    g = golden("comp_sedov_64_020")
    f = g["final"][4:-4, 4:-4]
    assert float(g["t"]) == 0.009286102192696327
    assert g["dts"][-1] == 0.000788786465650361
    assert abs(f[..., 1].sum() - 4774.750655256859) < 1e-9
    assert f[..., 0].max() == 1.9139231351538135 and f[..., 0].min() == 0.051270183038480036
    a = golden("adv_smooth_64")
    fa = a["final"][4:-4, 4:-4]
    fa = fa[..., 0] if fa.ndim == 3 else fa
    assert int(a["n"]) == 81
    assert abs(fa.sum() - 4310.466040637316) < 1e-9 and abs(fa.max() - 1.9600687314173393) < 1e-14


@pytest.mark.parametrize("k", range(4))
def test_comp_hllc_lm(golden, k):
    """the low-Mach HLLC variant (riemann_hllc_lowspeed,
    riemann.py:863-1020) against dumps of the reference's own functions; its
    scalar x**2 is libm pow under the shim (orc.set_scalar_pow)"""
    g = golden("comp_stages_lm")
    bcs = [str(b) for b in g[f"c{k}_bc"]]
    P, cfl = meta_to_params(g[f"c{k}_meta"], bcs, riemann="HLLC_lm")
    orc.set_scalar_pow(1)
    try:
        U = g[f"c{k}_U0"].copy()
        if "hse" in bcs:
            pass   # ghost cells of U0 are already filled by the reference
        rc, st = orc.comp_step(U, P, float(g[f"c{k}_dt"]), stages=True)
    finally:
        orc.set_scalar_pow(0)
    assert rc == 0
    for nm in ("FxT", "FyT", "Fx0", "Fy0", "Fx", "Fy"):
        assert max_rel_err(st[nm], g[f"c{k}_{nm}"]) == 0.0, (k, nm)
    ng = int(g[f"c{k}_meta"][2])
    assert np.array_equal(U[ng:-ng, ng:-ng], g[f"c{k}_U1"][ng:-ng, ng:-ng])


def _ramp_fill(U, P, bcs, dom, t):
    rp = orc.ramp_params(P.nx, P.ny, P.ng, dom[0], dom[1], dom[2], dom[3], P.gamma, t)
    orc.comp_fill_bc_ramp(U, P.nx, P.ny, P.ng, bcs, rp)


def oracle_ramp_run(g, nsteps):
    from helpers import DtPolicy
    bcs = [str(b) for b in g["bc"]]
    P, cfl = meta_to_params(g["meta"], bcs)
    f0, mx = g["drv"]
    U = g["ic"].copy()
    pol = DtPolicy(1.e30, f0, mx)
    dts = []
    for _ in range(nsteps):
        _ramp_fill(U, P, bcs, g["domain"], pol.t)
        dt = pol(orc.comp_dt(U, P.nx, P.ny, P.ng, P.dx, P.dy, P.gamma, cfl))
        rc, _ = orc.comp_step(U, P, dt)
        assert rc == 0
        pol.advance(dt)
        dts.append(dt)
    return U, np.array(dts), pol.t, P, bcs


def test_oracle_ramp(golden):
    """double Mach reflection with the time-dependent "ramp" boundary
    (compressible/BC.py:178-296): run and final ghost fill vs the reference"""
    g = golden("comp_ramp")
    U, dts, t, P, bcs = oracle_ramp_run(g, len(g["dts"]))
    assert np.array_equal(dts, g["dts"]) and t == float(g["t"])
    assert np.array_equal(U, g["final"])
    _ramp_fill(U, P, bcs, g["domain"], t)
    assert np.array_equal(U, g["filled"])


def _heat_case(g, k):
    pre = f"c{k}_"
    bcs = [str(b) for b in g[pre + "bc"]]
    sp = g[pre + "sponge"]
    over = dict(heating=(float(g[pre + "e_rate"]), g[pre + "prof"]),
                small_dens=float(g[pre + "small_dens"]))
    if sp[0]:
        over["sponge"] = tuple(sp[1:])
    return pre, bcs, over


@pytest.mark.parametrize("k", range(3))
def test_oracle_problem_sources(golden, k):
    """the problem source of heating / plume / convection
    (S[E] += rho e_rate exp(-(dist/r)^2); convection also has gravity, the
    sponge, a reflecting wall and the ambient boundary): stages of one step
    and a short run against the reference"""
    from helpers import oracle_comp_run
    g = golden("comp_heating")
    pre, bcs, over = _heat_case(g, k)
    meta = g[pre + "meta"]
    ng = int(meta[2])
    I = (slice(ng, -ng), slice(ng, -ng))
    P, cfl = meta_to_params(meta, bcs, **over)
    U = g[pre + "U0"].copy()
    rc, st = orc.comp_step(U, P, float(g[pre + "dt"]), stages=True)
    assert rc == 0
    for nm in ("Uxl0", "Uyr0", "Fx", "Fy"):
        assert np.array_equal(st[nm], g[pre + nm]), nm
    assert np.array_equal(U[I], g[pre + "U1"][I])
    f0, mx = g[pre + "drv"]
    U, dts, _ = oracle_comp_run(g[pre + "ic"], meta, bcs, 1.e30, len(g[pre + "dts"]), f0, mx,
                                ambient=tuple(g[pre + "ambient"]), **over)
    assert np.array_equal(dts, g[pre + "dts"])
    assert np.array_equal(U[I], g[pre + "final"][I])


# ---------------------------------------------------------------------------
# row f4: incompressible_viscous (lid-driven cavity)
# ---------------------------------------------------------------------------
def visc_bcs(names):
    """(bc_u, bc_v, bc_phi) names for the mesh boundary names of a viscous run
    (incompressible/simulation.py:33-48)"""
    names = [str(b) for b in names]
    phi = names if names[0] == "periodic" else ["neumann"] * 4
    return dict(bc_u=names, bc_v=names, bc_phi=phi)


def oracle_visc_run(ic2, meta, bcnames, nsteps=None, tmax=1.e30):
    from helpers import DtPolicy
    nx, ng, lim, proj, cfl, f0, mx, nu = meta
    nx, ng, lim, proj = int(nx), int(ng), int(lim), int(proj)
    bcs = visc_bcs(bcnames)
    q = nx + 2 * ng
    D = np.zeros((6, q, q))
    D[:2] = ic2
    orc.incomp_set_viscous(nu)
    try:
        orc.incomp_preevolve(D, nx, ng, cfl, lim, proj, **bcs)
        after_pre = D.copy()
        pol = DtPolicy(tmax, f0, mx)
        dts = []
        while pol.t < tmax and (nsteps is None or pol.n < nsteps):
            for n in range(6):
                codes = orc.bc_codes(bcs["bc_u"] if n < 2 else bcs["bc_phi"])
                orc.fill_ghost(D[n], nx, nx, ng, codes)
                if n < 2 and codes[3] == 8:
                    D[n][:, ng + nx:] = 1.0 if n == 0 else 0.0     # moving lid
            dt = pol(orc.bg_dt(D[0], D[1], nx, nx, ng, 1.0 / nx, 1.0 / nx, cfl))
            orc.incomp_step(D, nx, ng, dt, lim, proj, **bcs)
            pol.advance(dt)
            dts.append(dt)
    finally:
        orc.incomp_set_viscous(None)
    return D, after_pre, np.array(dts), pol


@pytest.mark.parametrize("k", range(3))
def test_oracle_incompressible_viscous(golden, k):
    g = golden("incomp_viscous")
    pre = f"i{k}_"
    meta = g[pre + "meta"]
    nx, ng = int(meta[0]), int(meta[1])
    D, after_pre, dts, _ = oracle_visc_run(g[pre + "ic"][:2], meta, g[pre + "bc"],
                                           nsteps=len(g[pre + "dts"]))
    assert np.abs(after_pre - g[pre + "after_pre"]).max() < 1e-13
    assert np.abs(dts / g[pre + "dts"] - 1).max() < 1e-12
    I = (slice(None), slice(ng, -ng), slice(ng, -ng))
    assert np.abs(D[I] - g[pre + "final"][I]).max() < 1e-11
    # one step from the reference's state with its dt: bit-identical pieces
    D = np.ascontiguousarray(g[pre + "U0"])
    orc.incomp_set_viscous(meta[7])
    try:
        st = orc.incomp_step(D, nx, ng, float(g[pre + "dt"]), int(meta[2]), int(meta[3]),
                             stages=True, **visc_bcs(g[pre + "bc"]))
    finally:
        orc.incomp_set_viscous(None)
    F = (slice(ng, ng + nx + 1), slice(ng, ng + nx))
    assert np.abs(st["umac"][F] - g[pre + "umac"][F]).max() < 1e-12
    assert np.abs(D[I] - g[pre + "U1"][I]).max() < 1e-11


def test_incompressible_viscous_reference_regression_cavity(golden):
    """pyro/test.py:111: incompressible_viscous cavity inputs.cavity vs
    cavity_n64_Re400_0025.h5 (64^2, Re 400, 25 steps, 4 MG solves per step)"""
    g = golden("incomp_cavity_0025")
    D, _, dts, pol = oracle_visc_run(g["ic"], g["meta"], g["bc"], nsteps=25,
                                     tmax=float(g["tmax"]))
    assert pol.n == int(g["nsteps"]) == 25 and abs(pol.t - float(g["t"])) < 1e-13
    ng = int(g["meta"][1])
    I = (slice(ng, -ng), slice(ng, -ng))
    assert np.abs(D[0][I] - g["gold"][0]).max() < 1e-10
    assert np.abs(D[1][I] - g["gold"][1]).max() < 1e-10
    assert np.abs(D[0][I] - g["run"][0]).max() < 1e-11


# ---------------------------------------------------------------------------
# row f4: compressible solver on a SphericalPolar grid
# ---------------------------------------------------------------------------
def nan_rel_err(a, b):
    """max relative error where both are finite; NaNs (the reflect-odd ghost
    faces of the reference hold sqrt(negative)) must sit at the same places"""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb)
    return max_rel_err(np.where(na, 0.0, a), np.where(nb, 0.0, b))


def sph_geom(g, pre):
    names = ("Lx", "Ly", "Ax", "Ay", "V", "dlogAx", "dlogAy", "x2d", "sint", "sinb", "sinc")
    dom = g[pre + "g_domain"]
    return orc.Geom({n: g[pre + "g_" + n] for n in names}, dom[0], dom[2])


def oracle_sph_run(g, pre, nsteps):
    from helpers import DtPolicy
    bcs = [str(b) for b in g[pre + "bc"]]
    P, cfl = meta_to_params(g[pre + "meta"], bcs, riemann="CGF")
    geom = sph_geom(g, pre)
    f0, mx = g[pre + "drv"]
    fix = 0.005 if str(g[pre + "problem"]) == "advect" else -1.0
    U = g[pre + "ic"].copy()
    pol = DtPolicy(1.e30, f0, mx, fix_dt=fix)
    dts = []
    for _ in range(nsteps):
        orc.comp_fill_bc(U, P.nx, P.ny, P.ng, bcs, P.gamma, P.grav, P.dy, (0.0,) * 4)
        dt = pol(orc.comp_dt_geom(U, P.nx, P.ny, P.ng, geom, P.gamma, cfl))
        rc, _ = orc.comp_step(U, P, dt, geom=geom)
        assert rc == 0
        pol.advance(dt)
        dts.append(dt)
    return U, np.array(dts)


@pytest.mark.parametrize("k", range(3))
def test_oracle_spherical(golden, k):
    """SphericalPolar geometry (mesh/patch.py:242-312): area / volume weighted
    update, geometric terms in the tracing and the sources, pressure gradients
    outside the fluxes, CGF interface states -- against dumps of the reference's
    own functions and a short run"""
    g = golden("comp_spherical")
    pre = f"c{k}_"
    bcs = [str(b) for b in g[pre + "bc"]]
    P, cfl = meta_to_params(g[pre + "meta"], bcs, riemann="CGF")
    geom = sph_geom(g, pre)
    ng = P.ng
    I = (slice(ng, -ng), slice(ng, -ng))
    orc.set_scalar_pow(1)
    try:
        U = g[pre + "U0"].copy()
        assert abs(orc.comp_dt_geom(U, P.nx, P.ny, ng, geom, P.gamma, cfl) /
                   float(g[pre + "dt"]) - 1) < 1e-14 or str(g[pre + "problem"]) == "advect"
        rc, st = orc.comp_step(U, P, float(g[pre + "dt"]), stages=True, geom=geom)
        assert rc == 0
        for nm in ("Uxl0", "Uxr0", "Uyl0", "Uyr0", "FxT", "FyT", "Uxl", "Uxr", "Uyl", "Uyr",
                   "Fx0", "Fy0", "avx", "avy", "Fx", "Fy"):
            assert nan_rel_err(st[nm], g[pre + nm]) < 1e-13, (k, nm, nan_rel_err(st[nm], g[pre + nm]))
        assert max_rel_err(U[I], g[pre + "U1"][I]) < 1e-13
        U, dts = oracle_sph_run(g, pre, len(g[pre + "dts"]))
    finally:
        orc.set_scalar_pow(0)
    assert np.abs(dts / g[pre + "dts"] - 1).max() < 1e-12
    assert max_rel_err(U[I], g[pre + "after"][I]) < 1e-11


# ---------------------------------------------------------------------------
# burgers_viscous: unsplit Burgers fluxes + one Helmholtz solve per component
# ---------------------------------------------------------------------------
def oracle_bgv_run(g, pre, nsteps):
    from helpers import DtPolicy
    nx, ng, lim, eps, cfl, f0, mx, fix, tmax = g[pre + "meta"]
    nx, ng, lim = int(nx), int(ng), int(lim)
    bcs = [str(b) for b in g[pre + "bc"]]
    codes = orc.bc_codes(bcs)
    U = g[pre + "ic"].copy()
    pol = DtPolicy(tmax, f0, mx, fix_dt=fix)
    dts = []
    for _ in range(nsteps):
        for n in range(2):
            orc.fill_ghost(U[n], nx, nx, ng, codes)
        dt = pol(orc.bg_dt(U[0], U[1], nx, nx, ng, 1.0 / nx, 1.0 / nx, cfl))
        orc.bgv_step(U[0], U[1], nx, ng, dt, lim, eps, bc_u=bcs, bc_v=bcs)
        pol.advance(dt)
        dts.append(dt)
    return U, np.array(dts)


@pytest.mark.parametrize("k", range(3))
def test_oracle_burgers_viscous(golden, k):
    """pyro/burgers_viscous/simulation.py:9-89 + interface.py:27-171 against runs
    of the reference: one step from a reference state and a short run"""
    g = golden("burgers_viscous")
    pre = f"v{k}_"
    nx, ng, lim, eps = (g[pre + "meta"][i] for i in range(4))
    nx, ng, lim = int(nx), int(ng), int(lim)
    bcs = [str(b) for b in g[pre + "bc"]]
    U = g[pre + "U0"].copy()
    orc.bgv_step(U[0], U[1], nx, ng, float(g[pre + "dt"]), lim, eps, bc_u=bcs, bc_v=bcs)
    I = (slice(None), slice(ng, -ng), slice(ng, -ng))
    assert np.abs(U[I] - g[pre + "U1"][I]).max() < 1e-13
    U, dts = oracle_bgv_run(g, pre, len(g[pre + "dts"]))
    assert np.abs(dts / g[pre + "dts"] - 1).max() < 1e-12
    assert np.abs(U[I] - g[pre + "final"][I]).max() < 1e-12


# ------------------------------------------------------- compressible_fv4 rhs
FV4_CASES = [("comp_fv4_rhs", c) for c in ("pulse", "sod", "rt")] + \
            [("comp_fv4_edges", c) for c in ("sodx", "rt", "heating", "quad", "pulse_dy")]


def fv4_oracle_params(g, case):
    """orc.comp_params of a comp_fv4_* fixture case (meta, small_dens, heating)"""
    U, meta = g[f"{case}_U"], g[f"{case}_meta"]
    dx, dy, gamma, grav, flat, sponge, rb, rf, tau = meta
    sd = float(g[f"{case}_small_dens"]) if f"{case}_small_dens" in g else -1.e200
    heat = (float(g[f"{case}_heat_rate"]), g[f"{case}_heat"]) if f"{case}_heat" in g else None
    return orc.comp_params(U.shape[0] - 8, U.shape[1] - 8, 4, dx, dy, gamma=gamma, use_flattening=int(flat),
                           grav=grav, small_dens=sd, sponge=(rb, rf, tau) if sponge else None, heating=heat)


@pytest.mark.parametrize("name,case", FV4_CASES, ids=[f"{n}-{c}" for n, c in FV4_CASES])
def test_oracle_fv4_rhs(golden, name, case):
    """orc_fv4_rhs against compressible_fv4 Simulation.substep / fluxes.fluxes of the reference:
    interior k, F_x and F_y on the whole array (zero where the reference writes nothing) and,
    where stored, the stage state after the call (clean_state floors the interior only).
    Bit for bit with both readings of the njit riemann_prim's scalar c**2 (x*x as numba
    compiles it, libm pow as the interpreted shim that made the fixtures evaluates it):
    they agree on every face of these cases."""
    g = golden(name)
    assert case in [str(c) for c in g["cases"]]
    I = (slice(4, -4), slice(4, -4))
    for scalar_pow in (0, 1):
        orc.set_scalar_pow(scalar_pow)
        try:
            U = g[f"{case}_U"].copy()
            rc, k, Fx, Fy = orc.fv4_rhs(U, fv4_oracle_params(g, case), fluxes=True)
        finally:
            orc.set_scalar_pow(0)
        assert rc == 0
        assert np.array_equal(k[I], g[f"{case}_k"][I]), scalar_pow
        assert np.array_equal(Fx, g[f"{case}_Fx"]), scalar_pow
        assert np.array_equal(Fy, g[f"{case}_Fy"]), scalar_pow
        if f"{case}_Uout" in g:
            assert np.array_equal(U, g[f"{case}_Uout"])
    if case == "sodx":       # the floor fired in the interior and left ghosts below it
        sd = float(g["sodx_small_dens"])
        assert (g["sodx_U"][I][..., 0] < sd).any() and (g["sodx_Uout"][..., 0] < sd).any()


def test_oracle_fv4_rhs_assert():
    """the two cons_to_prim asserts of fluxes.py:80-81: rc = 1 on a negative interior density
    or pressure, rc = 0 when only a ghost cell is bad"""
    nx, ny = 6, 5
    U = np.zeros((nx + 8, ny + 8, 4))
    U[..., 0], U[..., 1] = 1.0, 2.5
    P = orc.comp_params(nx, ny, 4, 0.1, 0.1)
    assert orc.fv4_rhs(U.copy(), P)[0] == 0
    for (i, j, n, v), rc in (((5, 6, 0, -1.0), 1), ((7, 4, 1, -3.0), 1), ((1, 6, 1, -3.0), 0)):
        V = U.copy()
        V[i, j, n] = v
        assert orc.fv4_rhs(V, P)[0] == rc, (i, j, n)


# ------------------------------------------- method-of-lines and nonuniform advection
ADVMOL_FILES = {"advrk_stages": ("start", "a_x", "a_y", "F_x", "F_y", "k"),
                "advweno_stages": ("start", "fpr_x", "fpr_y", "F_x", "F_y", "k")}


def advmol_case(g, k):
    """a recorded evolve() of advrk_stages.npz / advweno_stages.npz as the oracle's arguments"""
    pre = f"c{k}_"
    m = g[pre + "meta"]
    c = dict(nx=int(m[0]), ny=int(m[1]), ng=int(m[2]), par=int(m[3]), scheme=int(m[4]), dx=float(m[5]),
             dy=float(m[6]), u=float(m[7]), v=float(m[8]), ns=int(m[10]), method=str(g[pre + "method"]),
             bc=[str(b) for b in g[pre + "bc"]], dt=float(g[pre + "dt"]))
    c["alpha"] = float(m[11]) if c["scheme"] == 5 else 0.0
    return c


def advmol_oracle_step(c, a, stages=False):
    return orc.advmol_step(a, c["nx"], c["ny"], c["ng"], c["bc"], c["dx"], c["dy"], c["u"], c["v"],
                           c["scheme"], c["par"], c["method"], c["dt"], alpha=c["alpha"], stages=stages)


def advmol_slices(c):
    """where the device tests compare the planes of a stage: the faces the update reads (the
    fourth-order fluxes read face averages one face sideways)"""
    ng, nx, ny = c["ng"], c["nx"], c["ny"]
    t = 1 if c["scheme"] == 4 else 0
    return {"start": np.s_[:, :], "a_x": np.s_[ng:ng + nx + 1, ng - t:ng + ny + t],
            "a_y": np.s_[ng - t:ng + nx + t, ng:ng + ny + 1], "F_x": np.s_[ng:ng + nx + 1, ng:ng + ny],
            "F_y": np.s_[ng:ng + nx, ng:ng + ny + 1], "k": np.s_[ng:ng + nx, ng:ng + ny]}


@pytest.mark.parametrize("k", range(14))
@pytest.mark.parametrize("name", sorted(ADVMOL_FILES))
def test_oracle_advmol_stages(golden, name, k):
    """orc_advmol_step against one recorded evolve() of advection_rk / advection_fv4 /
    advection_weno: every stage's start with its ghost frame, face values, fluxes and k, and the
    new level with its ghost frame, bit for bit, from a plane whose ghost cells hold junk"""
    g = golden(name)
    assert int(g["ncases"]) == 14
    c = advmol_case(g, k)
    a = g[f"c{k}_Uin"].copy()
    st = advmol_oracle_step(c, a, stages=True)
    assert len(st) == c["ns"]
    sl = advmol_slices(c)
    for s in range(c["ns"]):
        for key, okey in zip(ADVMOL_FILES[name], orc.ADVMOL_PLANES):
            assert np.array_equal(st[s][okey][sl[okey]], g[f"c{k}_s{s}_{key}"][sl[okey]]), (s, key)
    assert np.array_equal(a, g[f"c{k}_new"])


def _smooth_to_t1(scheme, par, cfl=0.8, nx=32, ng=4, tmax=1.0):
    """inputs.smooth to t = 1 as the driver runs it: the Gaussian of advection/problems/smooth.py
    on the cell centres of mesh/patch.py:124-137 (advection_fv4: preevolve turns them into
    averages, fv.py:32-39), the time step of advection_rk/simulation.py:30-46 under
    simulation_null.compute_timestep"""
    dx = (1.0 - 0.0) / nx
    q = nx + 2 * ng
    x = 0.5 * (((np.arange(q) - ng) * dx + 0.0) + ((np.arange(q) + 1.0 - ng) * dx + 0.0))
    X, Y = np.meshgrid(x, x, indexing="ij")
    a = np.ascontiguousarray(1.0 + np.exp(-60.0 * ((X - 0.5)**2 + (Y - 0.5)**2)))
    bc = ["periodic"] * 4
    u = v = 1.0
    if scheme == 4:
        orc.fill_ghost(a, nx, nx, ng, bc)
        c = a[ng:-ng, ng:-ng]
        lap = (a[ng - 1:-ng - 1, ng:-ng] - 2 * c + a[ng + 1:q - ng + 1, ng:-ng]) / dx**2 + \
              (a[ng:-ng, ng - 1:-ng - 1] - 2 * c + a[ng:-ng, ng + 1:q - ng + 1]) / dx**2
        a[ng:-ng, ng:-ng] = c + dx**2 * lap / 24.0
    t, n = 0.0, 0
    while t < tmax:
        dt = cfl / (max(abs(u), 1e-12) / dx + max(abs(v), 1e-12) / dx)
        if t + dt > tmax:
            dt = tmax - t
        orc.advmol_step(a, nx, nx, ng, bc, dx, dx, u, v, scheme, par, "RK4", dt, alpha=float(np.sqrt(u**2 + v**2)))
        t += dt
        n += 1
    return a[ng:-ng, ng:-ng], n, t


@pytest.mark.parametrize("scheme,par,name,key", [(2, 2, "advrk_regress", "s2_"), (4, 2, "advrk_regress", "s4_"),
                                                 (5, 2, "advweno_regress", "o2_"), (5, 3, "advweno_regress", "o3_")])
def test_oracle_advmol_regression_smooth(golden, scheme, par, name, key):
    """the 81 steps of the reference's regression runs (pyro/test.py: advection_rk,
    advection_fv4, advection_weno `smooth`), bit for bit"""
    g = golden(name)
    a, n, t = _smooth_to_t1(scheme, par)
    nref, tref = (g[key + "meta"][:2]) if scheme == 5 else (g[key + "n"], g[key + "t"])
    assert (n, t) == (81, 1.0) and (int(nref), float(tref)) == (81, 1.0)
    assert np.array_equal(a, g[key + "density"])


@pytest.mark.parametrize("k", range(7))
def test_oracle_advnu_stages(golden, k):
    """orc_advnu_step against one recorded fill_BC_all + evolve() of advection_nonuniform: the
    whole scratch planes a_x, a_y, F_x, F_y and the new density with its ghost frame, bit for
    bit, from planes whose ghost cells hold junk; the velocity planes are left alone"""
    g = golden("advnu_stages")
    assert int(g["ncases"]) == 7
    pre = f"c{k}_"
    m = g[pre + "meta"]
    nx, ny, ng, lim = (int(x) for x in m[:4])
    U = g[pre + "Uin"]                       # x-velocity, y-velocity, x-shift, y-shift, density
    bc = [[str(b) for b in row] for row in g[pre + "bc"]]
    a, u, v = U[4].copy(), U[0].copy(), U[1].copy()
    d = orc.advnu_step(a, u, v, nx, ny, ng, [bc[4], bc[0], bc[1]], float(m[4]), float(m[5]),
                       float(g[pre + "dt"]), lim, stages=True)
    for n, key in enumerate(("a_x", "a_y", "F_x", "F_y")):
        assert np.array_equal(d[n], g[pre + key]), key
    assert np.array_equal(a, g[pre + "new"])
    assert np.array_equal(u, U[0]) and np.array_equal(v, U[1])


def test_oracle_pow2_is_the_library_call():
    """orc_pow2 is pow(x, 2.0) of this host's C library (math.pow is the same call), not a
    product the compiler folded it into"""
    import math
    rng = np.random.default_rng(5)
    x = np.concatenate([10.0 ** rng.uniform(-100, 100, 200000) * rng.choice([-1.0, 1.0], 200000),
                        [0.0, -0.0, 1.0, -1.0, 1e150, 1e-200]])
    got = orc.pow2(x)
    assert np.array_equal(got, np.array([math.pow(float(t), 2.0) for t in x]))
    assert np.count_nonzero(got != x * x) > 0
