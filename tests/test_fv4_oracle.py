"""k_fv4_rhs (pyrohip_comp_fv4_rhs) against the C oracle orc_fv4_rhs (oracle/pyro_oracle.c,
pinned to the reference by tests/test_oracle_golden.py) over grid shapes around the kernel's
8 x 32 tiles (x rows by y columns) and over states that reach the scheme's edges: jumps on and
next to tile seams, densities below small_dens, near-vacuum cells, ghost cells that are not
boundary-consistent.  Each call writes into slot 1 of a three-slot k state filled with a
sentinel; the interior k is compared with the oracle, everything else of k must keep the
sentinel, and the stage state may change only by the interior density floor.

Also: the two small fv4 kernels (k_from_centers, k_sdc_update) at ragged block sizes against
numpy in their operation order, and the refusal of k == y.

The `dev` tests run on the emulated build here and on the MI355X under -m gpu (with the
larger grids: many tiles, a short-wide grid and one taller than 65535 rows)."""
import numpy as np
import pytest

from oracle import orc

TI, TJ = 8, 32          # the kernel's tile (comp_fv4.hip)
NG = 4
SENTINEL = 7.25
TOL = {0: 1e-13, 1: 1e-10}


def _prim_to_cons(r, u, v, p, gamma):
    return np.stack([r, p / (gamma - 1.0) + 0.5 * r * (u * u + v * v), r * u, r * v], axis=-1)


def make_state(kind, nx, ny, gamma, seed):
    """a cell-average state (qx, qy, 4) over the whole array: the ghost cells hold arbitrary
    valid values, not boundary-consistent ones"""
    rng = np.random.default_rng(seed)
    qx, qy = nx + 2 * NG, ny + 2 * NG
    X, Y = np.meshgrid(np.arange(qx) / qx, np.arange(qy) / qy, indexing="ij")
    if kind in ("smooth", "floor"):
        ph = rng.random(6) * 2 * np.pi
        r = 1.0 + 0.4 * np.sin(2 * np.pi * X + ph[0]) * np.cos(2 * np.pi * Y + ph[1]) + 0.05 * rng.random((qx, qy))
        u = 0.5 * np.sin(2 * np.pi * Y + ph[2]) + 0.05 * rng.standard_normal((qx, qy))
        v = 0.5 * np.cos(2 * np.pi * X + ph[3]) + 0.05 * rng.standard_normal((qx, qy))
        p = 1.0 + 0.3 * np.cos(2 * np.pi * (X + Y) + ph[4]) + 0.05 * rng.random((qx, qy))
        if kind == "floor":
            # single cells and small patches below small_dens (0.05), interior and ghosts
            m = rng.random((qx, qy)) < 0.08
            m[0, 0] = m[NG, NG] = m[-1, NG + 1] = m[NG + 1, -2] = True
            r = np.where(m, 0.01 + 0.03 * rng.random((qx, qy)), r)
    elif kind == "blocks":
        # piecewise-constant blocks whose jumps sit on the tile seams (i = ilo + 8m + {-1, 0, 1},
        # j = jlo + 32m + {-1, 0, 1}), shock-sized ratios
        cx = sorted({NG + TI * m + d for m in range((nx + TI - 1) // TI + 1) for d in (-1, 0, 1)})
        cy = sorted({NG + TJ * m + d for m in range((ny + TJ - 1) // TJ + 1) for d in (-1, 0, 1)})
        bi = np.searchsorted(cx, np.arange(qx), side="right")
        bj = np.searchsorted(cy, np.arange(qy), side="right")
        states = np.array([[1.0, 0.0, 0.0, 1.0], [0.125, 0.0, 0.0, 0.1], [5.0, -2.0, 1.5, 30.0],
                           [0.2, 3.0, -3.0, 0.05], [1.5, 1.0, 2.5, 0.5], [0.05, -1.0, 0.0, 0.02]])
        pick = rng.integers(0, len(states), size=(len(cx) + 1, len(cy) + 1))
        S = states[pick[bi][:, bj]]
        r, u, v, p = (S[..., n] for n in range(4))
    elif kind == "vacuum":
        # near-vacuum cells next to dense ones, and hot cells at rest inside converging cold
        # flow: the to_centers mask (c[0] < 0 or rhoe < 0) and the q_avg positivity fallback
        r = 1.0 + 0.2 * rng.random((qx, qy))
        u = 0.2 * rng.standard_normal((qx, qy))
        v = 0.2 * rng.standard_normal((qx, qy))
        p = 1.0 + 0.2 * rng.random((qx, qy))
        vac = rng.random((qx, qy)) < 0.06
        r = np.where(vac, 1e-6, r)
        p = np.where(vac, 1e-7, p)
        for _ in range(max(2, nx * ny // 60)):
            i, j = rng.integers(1, qx - 1), rng.integers(1, qy - 1)
            r[i - 1:i + 2, j - 1:j + 2] = 1.0
            p[i - 1:i + 2, j - 1:j + 2] = 1e-6
            u[i - 1, j], u[i + 1, j], u[i, j] = 5.8, -5.8, 0.0
            v[i, j - 1], v[i, j + 1] = 5.8, -5.8
            u[i, j - 1] = u[i, j + 1] = v[i - 1, j] = v[i + 1, j] = 0.0
            v[i, j] = 0.0
            p[i, j] = 1.0
    elif kind == "edges":
        # cubic profiles with an extremum in the first cell outside the interior and an
        # inflection next to it, so that the limiter of that cell reaches its d3a test with
        # four equal d3a values and the decision turns on what the reference leaves there:
        # the density, at the low x and y edges and the high x edge, against q_avg = 0 on the
        # outermost ring (fluxes.py:84-86); the x-velocity at the high y edge, 0 on the ring
        # as the cubic continues, against d3a = 0 past the y sweep's last cell
        # (fourth_order.py:175-178)
        def F(t):
            t = np.minimum(t, 6)
            return (t - 2.0)**3 - 3.0 * (t - 2.0)
        i, j = np.arange(qx)[:, None], np.arange(qy)[None, :]
        r = 1.0 + 0.01 * (F(i) + F(qx - 1 - i) + F(j)) + 0.0 * j
        u = 0.01 * (F(qy - 1 - j) + 2.0) + 0.0 * i
        v = np.full((qx, qy), -0.2)     # (inflow at the high y edge: its face takes u from above)
        p = np.ones((qx, qy))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(_prim_to_cons(r, u, v, p, gamma))


# (state, use_flattening, grav, gamma, dy / dx, sponge, heating, small_dens)
COMBOS = {
    "smooth": ("smooth", 1, 0.0, 1.4, 1.0, False, False, -1.e200),
    "seams": ("blocks", 1, -1.0, 5 / 3, 1.3, True, False, -1.e200),
    "seams_noflat": ("blocks", 0, 0.0, 1.4, 0.7, False, True, -1.e200),
    "floor": ("floor", 1, -1.0, 5 / 3, 1.0, False, True, 0.05),
    "vacuum": ("vacuum", 1, 0.0, 1.4, 1.0, True, False, -1.e200),
    "smooth_src": ("smooth", 0, -1.0, 5 / 3, 0.8, True, True, -1.e200),
    "edges": ("edges", 1, 0.0, 1.4, 1.0, False, False, -1.e200),
}
SPONGE = (1.2, 0.8, 0.05)      # rho_begin, rho_full, timescale: straddled by the states' densities


def run_case(ctx, nx, ny, combo, fast, seed=0, determinism=False):
    """the kernel and the oracle on one case: checks what k outside the slot's interior and the
    stage state hold (and, with determinism, a second call's bits); returns (per-variable rel.
    errors of the interior k against the oracle, oracle fallback counts)"""
    from pyro2_amd import device
    kind, flat, grav, gamma, aspect, sponge, heat, small = COMBOS[combo]
    qx, qy = nx + 2 * NG, ny + 2 * NG
    U0 = make_state(kind, nx, ny, gamma, seed=1000 * seed + nx * 7 + ny)
    dx = 1.0 / 64
    dy = aspect * dx
    rng = np.random.default_rng(seed + 17)
    # (set_heating fills the profile's ghost cells by the energy's boundary rules, here
    # outflow: the profile's ghosts are the edge values, as the device holds them)
    prof = np.pad(rng.random((nx, ny)), NG, mode="edge") if heat else None
    rate = 0.7 if heat else 0.0

    Po = orc.comp_params(nx, ny, NG, dx, dy, gamma=gamma, use_flattening=flat, grav=grav,
                         small_dens=small, sponge=SPONGE if sponge else None,
                         heating=(rate, prof) if heat else None)
    Uo = U0.copy()
    rc, ko, counts = orc.fv4_rhs(Uo, Po, counts=True)
    assert rc == 0, "the case must be a valid state"

    P = device.make_comp_params(dx, dy, gamma=gamma, grav=grav, use_flattening=flat, fast_math=fast,
                                riemann="CGF", small_dens=small, sponge=SPONGE if sponge else None,
                                heat_rate=rate)
    s = device.DeviceState(ctx, nx, ny, 4, [["outflow"] * 4] * 4)
    s.upload(U0)
    if heat:
        s.set_heating(prof)
    k = device.DeviceState(ctx, nx, ny, 4, [["outflow"] * 4] * 12)
    k.upload(np.full((qx, qy, 12), SENTINEL))
    s.comp_fv4_rhs(P, k, 1)
    kall = k.download()
    I = (slice(NG, NG + nx), slice(NG, NG + ny))

    # 1. the interior of slot 1 against the oracle
    got = kall[..., 4:8]
    err = [float(np.abs(got[I][..., n] - ko[I][..., n]).max() / max(np.abs(ko[I][..., n]).max(), 1e-300))
           for n in range(4)]
    # 2. nothing else of k changed: slots 0 and 2, and the ghost frame of slot 1
    untouched = np.ones((qx, qy, 12), dtype=bool)
    untouched[I + (slice(4, 8),)] = False
    assert np.all(kall[untouched] == SENTINEL), "k changed outside the slot's interior"
    # 3. the stage state: the oracle's (the density floored on the interior, nothing else)
    Ud = s.download()
    want = U0.copy()
    want[I + (0,)] = np.where(U0[I + (0,)] < small, small, U0[I + (0,)])
    assert np.array_equal(Uo, want)
    assert np.array_equal(Ud, want), "the stage state changed beyond the interior density floor"
    # 4. determinism (GPU): the same input again gives the same bits
    if determinism:
        s.upload(U0)
        k.upload(np.full((qx, qy, 12), SENTINEL))
        s.comp_fv4_rhs(P, k, 1)
        assert np.array_equal(k.download(), kall), "a second call gave other bits"
    print(f"{nx}x{ny} {combo} {'fast' if fast else 'exact'} rel err {max(err):.3e} "
          f"bit-identical {bool(np.array_equal(got[I], ko[I]))} fallbacks {counts}")
    return err, counts


EMU_SHAPES = [(4, 4), (7, 31), (8, 32), (9, 33), (4, 70), (41, 5), (17, 65)]
# Cases whose interior k the contracted build (fast_math 1) on the MI355X is not held to 1e-10
# on, because a comparison whose two sides are equal in exact arithmetic is decided by round-off
# (the exact build is bit-identical or within 1e-16 on every one, and the contracted build keeps
# every other check there):
#   vacuum  flatten_multid's choice p[i+1] - p[i-1] > 0 (reconstruction.py:172-178) between two
#           cold cells of equal pressure 1e-6 whose q_bar pressure is E - kinetic energy with
#           the kinetic energy 1e4 times larger: xi of the cell between them is 0 or 1
#           (1.4e-2 .. 2.1e-2 of max |k|)
#   seams   the limiter's extremum test (a - a[i-2]) (a[i+2] - a) <= 0 (fourth_order.py:97-98)
#           with cells i and i-2 in one block, whose q_avg agree up to round-off (0.8e-7 ..
#           1.6e-7 of max |k|, in the density)
# A relative perturbation of 1e-15 of the state moves the oracle's own k by the same amounts.
FAST_K_TIES = {((4, 70), "vacuum"), ((17, 65), "vacuum"), ((2000, 9), "vacuum"), ((1021, 1999), "vacuum"),
               ((70000, 6), "vacuum"), ((2000, 9), "seams"), ((1021, 1999), "seams"), ((70000, 6), "seams")}


def _check_k(ctx, shape, combo, fast, err):
    if fast and ctx.kind == "hip" and (shape, combo) in FAST_K_TIES:
        return
    assert max(err) <= TOL[fast], (combo, err)


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("shape", EMU_SHAPES, ids=[f"{a}x{b}" for a, b in EMU_SHAPES])
def test_fv4_rhs_vs_oracle_shapes(dev, shape, fast):
    """every state / parameter combination on grids around one tile: the smallest grid the
    library accepts (nx = ny = ng = 4), one cell short of, at and one past a tile, below a
    tile in x with three y tiles, below a tile in y with six x tiles, and 3 x 3 ragged tiles"""
    nx, ny = shape
    for combo in COMBOS:
        err, counts = run_case(dev, nx, ny, combo, fast, determinism=dev.kind == "hip")
        _check_k(dev, shape, combo, fast, err)
        if combo == "vacuum" and nx * ny >= 100:
            assert counts[0] > 0 and counts[1] > 0, counts


TALL = (70000, 6)    # more than 65535 rows: the row index of k_fv4_prep, k_from_centers and
                     # k_sdc_update is blockIdx.y
GPU_CASES = [((1021, 1999), ("smooth", "seams", "vacuum")),   # many tiles, ragged both ways
             ((2000, 9), tuple(COMBOS)),                # 250 x-tiles below one y tile
             (TALL, ("smooth", "seams", "floor", "vacuum"))]


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("shape,combos", GPU_CASES, ids=[f"{a}x{b}" for (a, b), _ in GPU_CASES])
def test_fv4_rhs_vs_oracle_large(hip, shape, combos, fast):
    """the same checks on the MI355X over many tiles (where a missing barrier or an LDS union
    reused too early shows), a short-wide grid and a grid taller than 65535 rows.  On the tall
    grid the floor case only passes if k_fv4_prep ran over every row (k_fv4_rhs floors what it
    loads, so k alone cannot tell), and a bad density in row 69000 must be refused"""
    nx, ny = shape
    for combo in combos:
        err, _ = run_case(hip, nx, ny, combo, fast, determinism=True)
        _check_k(hip, shape, combo, fast, err)
    if shape == TALL:
        from pyro2_amd import device
        from pyro2_amd._lib import ERR_STATE, PyroHipError
        U = make_state("smooth", nx, ny, 1.4, seed=5)
        U[NG + 69000, NG + 2, 0] = -1.0
        s = device.DeviceState(hip, nx, ny, 4, [["outflow"] * 4] * 4)
        s.upload(U)
        k = device.DeviceState(hip, nx, ny, 4, [["outflow"] * 4] * 4)
        k.upload(np.full((nx + 2 * NG, ny + 2 * NG, 4), SENTINEL))
        P = device.make_comp_params(1 / 64, 1 / 64, riemann="CGF", fast_math=fast)
        with pytest.raises(PyroHipError) as ei:
            s.comp_fv4_rhs(P, k, 0)
        assert ei.value.code == ERR_STATE
        assert np.all(k.download() == SENTINEL)


def test_fv4_rhs_refuses_aliasing(dev):
    """k == y: the tiles would read cells that other tiles have already overwritten"""
    from pyro2_amd import device
    from pyro2_amd._lib import PyroHipError
    nx, ny = 9, 33
    U0 = make_state("smooth", nx, ny, 1.4, seed=3)
    s = device.DeviceState(dev, nx, ny, 4, [["outflow"] * 4] * 4)
    s.upload(U0)
    P = device.make_comp_params(1 / 64, 1 / 64, riemann="CGF")
    with pytest.raises(PyroHipError) as ei:
        s.comp_fv4_rhs(P, s, 0)
    assert ei.value.code == 10001 and "stage state" in str(ei.value)
    assert np.array_equal(s.download(), U0)


# ---------------------------------------------------------------- from_centers, SDC update
SMALL_SHAPES = [(4, 257), (4, 300), (5, 257), (9, 300)]     # ragged 256-wide blocks in y


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=[f"{a}x{b}" for a, b in SMALL_SHAPES])
def test_fv4_from_centers_ragged(dev, shape):
    """k_from_centers (FV2d.from_centers, fv.py:31-39) against numpy in the kernel's operation
    order, bit for bit: interior a + dx^2 lap(a) / 24 of the ghost-filled copy; the ghosts
    are those of the fill and the other variables (var = 2) stay as they were"""
    from pyro2_amd import device
    nx, ny = shape
    qx, qy = nx + 2 * NG, ny + 2 * NG
    rng = np.random.default_rng(nx * 1000 + ny)
    dx, dy = 0.3 / nx, 0.45 / nx
    bcs = [["outflow", "outflow", "reflect-even", "reflect-even"]] * 4
    for var in (2, -1):
        a0 = 1.0 + rng.random((qx, qy, 4))
        s = device.DeviceState(dev, nx, ny, 4, bcs)
        s.upload(a0)
        s.fill_bc()
        filled = s.download()
        s.from_centers(var, dx, dy)
        got = s.download()
        want = filled.copy()
        for n in (range(4) if var < 0 else (var,)):
            b = filled[..., n]
            c = b[NG:-NG, NG:-NG]
            lap = (b[NG - 1:-NG - 1, NG:-NG] - 2 * c + b[NG + 1:qx - NG + 1, NG:-NG]) / (dx * dx) + \
                  (b[NG:-NG, NG - 1:-NG - 1] - 2 * c + b[NG:-NG, NG + 1:qy - NG + 1]) / (dy * dy)
            want[NG:-NG, NG:-NG, n] = c + dx * dx * lap / 24.0
        assert np.array_equal(got, want), var


@pytest.mark.gpu
def test_fv4_from_centers_tall(hip):
    """k_from_centers on a grid taller than 65535 rows (the row index is blockIdx.y)"""
    test_fv4_from_centers_ragged(hip, TALL)


# (slot_new, slot_old, slots_q): the node updates of compressible_sdc/simulation.py:85-87
SDC_SLOTS = [(1, 0, (0, 1, 2)), (0, 1, (2, 0, 1)), (2, 2, (0, 1, 2)), (1, 2, (1, 1, 0))]


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=[f"{a}x{b}" for a, b in SMALL_SHAPES])
def test_fv4_sdc_update_ragged(dev, shape):
    """k_sdc_update against numpy in the kernel's operation order, bit for bit, for new/old
    swapped, slot_new == slot_old and repeated quadrature slots; the ghosts of dst keep what
    they held"""
    from pyro2_amd import device
    nx, ny = shape
    qx, qy = nx + 2 * NG, ny + 2 * NG
    rng = np.random.default_rng(nx + 7 * ny)
    I = (slice(NG, -NG), slice(NG, -NG))
    src0 = rng.standard_normal((qx, qy, 4))
    K = rng.standard_normal((qx, qy, 12))
    for dt in (0.0137, 1e-3):
        for sn, so, sq in SDC_SLOTS:
            cq = rng.standard_normal(3)
            dst0 = rng.standard_normal((qx, qy, 4))
            src = device.DeviceState(dev, nx, ny, 4, [["outflow"] * 4] * 4)
            dst = device.DeviceState(dev, nx, ny, 4, [["outflow"] * 4] * 4)
            k = device.DeviceState(dev, nx, ny, 4, [["outflow"] * 4] * 12)
            src.upload(src0)
            dst.upload(dst0)
            k.upload(K)
            dst.comp_sdc_update(src, k, sn, so, sq, cq, dt)
            ks = [K[..., 4 * m:4 * m + 4] for m in range(3)]
            idt, hdt = dt / 24.0, 0.5 * dt
            integral = idt * (cq[0] * ks[sq[0]] + cq[1] * ks[sq[1]] + cq[2] * ks[sq[2]])
            want = dst0.copy()
            want[I] = (src0 + hdt * (ks[sn] - ks[so]) + integral)[I]
            assert np.array_equal(dst.download(), want), (dt, sn, so, sq)
            assert np.array_equal(src.download(), src0) and np.array_equal(k.download(), K)


@pytest.mark.gpu
def test_fv4_sdc_update_tall(hip):
    """k_sdc_update on a grid taller than 65535 rows (the row index is blockIdx.y)"""
    test_fv4_sdc_update_ragged(hip, TALL)
