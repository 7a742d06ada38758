// Linear advection in a velocity field that varies from cell to cell, 2nd-order unsplit CTU
// update: ONE launch per time step.
//
// Replaces (reference file:line)
//   pyro/advection_nonuniform/simulation.py:64-118        method_compute_timestep, evolve
//   pyro/advection_nonuniform/advective_fluxes.py:1-127   unsplit_fluxes
//   pyro/mesh/reconstruction.py:9-120                     limit / limit2 / limit4
//   pyro/mesh/array_indexer.py:150-274                    fill_ghost of density, u and v
//
// Roofline: HBM bound, 32 B per cell update (read a, u, v, write a).
//
// The uniform kernel (advection.hip: k_adv_step) is specialised at compile time on the signs
// of ONE (u, v): which rows and lanes a state comes from is fixed.  Here the upwind side
// changes from cell to cell, so the kernel works on 2-d tiles in LDS, where a neighbour chosen
// at run time is an address and not a lane or a register:
//   1. a (4 cells of apron), u and v (2 cells) of a 16 x 32 tile are loaded THROUGH the ghost
//      fill's index maps, each with the boundary types of its own variable (the odd reflection
//      of the normal velocity is one of them), together with every cell's upwind offset;
//   2. the limited slopes in x and y, once per cell of the tile and its apron of 2;
//   3. the interface states a_x, a_y (per-cell Courant numbers, selects on the sign of the velocity);
//   4. the fluxes F_x, F_y with their transverse corrections (into the slopes' LDS);
//   5. the conservative update of the interior cells; ghost cells of the tile get the filled
//      value of the OLD level, which is what the reference's in-place update leaves there.
// The tiles cover the whole array, ghost frame included; nothing else writes the new plane.
//
// Contract.
//  * Ghost cells are never read from memory: density, u and v are taken from their interior
//    source cells by the boundary rules (outflow / reflect-even / reflect-odd / periodic), as
//    CellCenterData2d.fill_BC_all() at the start of the step would have stored them.
//  * The shift planes ("x-shift", "y-shift") are NOT read.  Simulation.initialize() stores
//    shift = -1 where the velocity is > 0, else 0, and fill_BC_all() then fills the shifts with the
//    boundary types of the velocities: the offset of an interior cell is that function of its
//    velocity, the offset of a ghost cell is the offset of its source cell, NEGATED where the
//    velocity's reflection is odd (there the reference's ghost cell holds -(-1) = +1: it looks
//    one cell further out; a zero stays zero).  That is what the kernel evaluates.  A caller that
//    puts anything else into the shift planes gets the reference's behaviour for THESE shifts.
//  * The interface states exist on the interior grown by one cell and are zero beyond it, as in
//    the reference's scratch arrays: the transverse flux difference of the face behind an oddly
//    reflecting side (offset +1: one cell further out) is taken from those zeros.
//  * u == 0 (and -0.0) takes the `else` branch of the reference (the + formula) with offset 0.
//
// Compiled twice (build.py): bit-faithful (-ffp-contract=off, the reference's operation order,
// cx = u*dt/dx as a product and a true division per cell: results identical to NumPy) and
// contracted (-ffp-contract=fast, cx = u*(dt/dx)); pyrohip_advnu_params.fast_math selects.
#include "builds.h"
#include "common.h"
#include "stencil.h"

namespace pyro {
namespace PYRO_NS {

// Tile geometry.  A cell's update reaches a at distance 3 where all offsets are 0 / -1 and at
// distance 4 behind an oddly reflecting side (offset +1 in the first ghost cell): apron NU_HA.
// Slopes, velocities, offsets, states and fluxes live on the tile grown by NU_HB.
constexpr int NU_TI = 16, NU_TJ = 32, NU_HA = 4, NU_HB = 2, NU_THREADS = 256;
constexpr int NU_AH = NU_TI + 2 * NU_HA, NU_AW = NU_TJ + 2 * NU_HA;
constexpr int NU_BH = NU_TI + 2 * NU_HB, NU_BW = NU_TJ + 2 * NU_HB;
constexpr int NU_D = NU_HA - NU_HB;      // B index + NU_D = A index

struct AdvNuParams {
    double dt, dx, dy;
    double dtdx, dtdy;      // dt/dx, dt/dy              simulation.py:92-93
    double dtdx2, dtdy2;    // 0.5*dt/dx, 0.5*dt/dy      advective_fluxes.py:114-115
    int gx, gy;             // tiles across (columns) / down (rows)
    int bc[12];             // xl, xr, yl, yr of the density, u, v
};

// index of a cell in the slopes' / velocities' LDS array -> its index in the array of a
__device__ __forceinline__ int nu_b2a(int k)
{
    const int r = k / NU_BW, c = k - r * NU_BW;
    return (r + NU_D) * NU_AW + c + NU_D;
}

template <int LIM>
__global__ __launch_bounds__(NU_THREADS) void k_advnu_step(const double *__restrict__ ain,
                                                           const double *__restrict__ uin,
                                                           const double *__restrict__ vin,
                                                           double *__restrict__ aout, Geom g, AdvNuParams P,
                                                           double *__restrict__ dump)
{
    __shared__ double A[NU_AH * NU_AW];
    __shared__ double U[NU_BH * NU_BW], V[NU_BH * NU_BW];
    __shared__ double SX[NU_BH * NU_BW], SY[NU_BH * NU_BW];      // slopes, then F_x / F_y
    __shared__ double AX[NU_BH * NU_BW], AY[NU_BH * NU_BW];
    __shared__ int SU[NU_BH * NU_BW], SV[NU_BH * NU_BW];         // upwind offsets in x / y
    int bx, by;
    if (!xcd_block_2d(P.gx, P.gy, bx, by)) return;
    const int I0 = by * NU_TI, J0 = bx * NU_TJ;                  // first array cell of the tile
    const int tid = threadIdx.x;

    // ---- 1. loads through the ghost fill
    {
        const BcMap mr = bc_map(g.ilo, g.ihi, g.ng, P.bc[0], P.bc[1], true);
        const BcMap mc = bc_map(g.jlo, g.jhi, g.ng, P.bc[2], P.bc[3], true);
        for (int n = tid; n < NU_AH * NU_AW; n += NU_THREADS) {
            const int r = n / NU_AW, c = n - r * NU_AW;
            const TileSrc s = tile_src(g, mr, mc, I0 + r - NU_HA, J0 + c - NU_HA);
            const double raw = ain[s.off];
            A[n] = s.neg ? -raw : raw;
        }
        const BcMap ur = bc_map(g.ilo, g.ihi, g.ng, P.bc[4], P.bc[5], true);
        const BcMap uc = bc_map(g.jlo, g.jhi, g.ng, P.bc[6], P.bc[7], true);
        const BcMap vr = bc_map(g.ilo, g.ihi, g.ng, P.bc[8], P.bc[9], true);
        const BcMap vc = bc_map(g.jlo, g.jhi, g.ng, P.bc[10], P.bc[11], true);
        for (int n = tid; n < NU_BH * NU_BW; n += NU_THREADS) {
            const int r = n / NU_BW, c = n - r * NU_BW;
            const int i = I0 + r - NU_HB, j = J0 + c - NU_HB;
            // offset of the source cell (simulation.py:18-26), negated with an odd reflection
            const TileSrc su = tile_src(g, ur, uc, i, j);
            const double ru = uin[su.off];
            const int ou = (ru > 0.0) ? -1 : 0;
            U[n] = su.neg ? -ru : ru;
            SU[n] = su.neg ? -ou : ou;
            const TileSrc sv = tile_src(g, vr, vc, i, j);
            const double rv = vin[sv.off];
            const int ov = (rv > 0.0) ? -1 : 0;
            V[n] = sv.neg ? -rv : rv;
            SV[n] = sv.neg ? -ov : ov;
        }
    }
    __syncthreads();

    // ---- 2. limited slopes (reconstruction.limit), one pair per cell.  The reference's limit2 is
    // zero beyond the interior grown by two cells, and limit4 takes its neighbours' limit2 as
    // stored: the slope of the second ghost cell (read behind an oddly reflecting side) is built
    // with a zero for the third one's
    auto slope = [&](double am2, double am1, double a0, double ap1, double ap2, bool lo, bool hi) {
        if (LIM == 0) return 0.5 * (ap1 - am1);
        if (LIM == 1) return limit2(am1, a0, ap1);
        const double l2m = lo ? limit2(am2, am1, a0) : 0.0;
        const double l2p = hi ? limit2(a0, ap1, ap2) : 0.0;
        return limit4_from(l2m, l2p, am1, a0, ap1);
    };
    for (int n = tid; n < NU_BH * NU_BW; n += NU_THREADS) {
        const int r = n / NU_BW, c = n - r * NU_BW;
        const int i = I0 + r - NU_HB, j = J0 + c - NU_HB;
        const int k = (r + NU_D) * NU_AW + c + NU_D;
        const double a0 = A[k];
        SX[n] = slope(A[k - 2 * NU_AW], A[k - NU_AW], a0, A[k + NU_AW], A[k + 2 * NU_AW],
                      i - 1 >= g.ilo - 2, i + 1 <= g.ihi + 2);
        SY[n] = slope(A[k - 2], A[k - 1], a0, A[k + 1], A[k + 2], j - 1 >= g.jlo - 2, j + 1 <= g.jhi + 2);
    }
    __syncthreads();

    // ---- 3. interface states on the lower faces (advective_fluxes.py:76-102): the upwind cell
    // is the cell itself or its neighbour at the offset; the sign of the velocity picks the formula
    auto state = [&](double vel, double courant, double a, double sl) {
        const bool neg = vel < 0.0;
        const double f = neg ? 1.0 + courant : 1.0 - courant;
        const double t = 0.5 * f * sl;
        return neg ? a - t : a + t;
    };
    // (the reference builds the states in scratch arrays on the interior grown by one cell:
    // beyond it they are zero, and the transverse term of the face behind an oddly reflecting
    // side -- offset +1 -- reads those zeros)
    auto in_buf1 = [&](int i, int j) {
        return i >= g.ilo - 1 && i <= g.ihi + 1 && j >= g.jlo - 1 && j <= g.jhi + 1;
    };
    // a_x: rows 0 .. NU_TI of the tile, columns -1 .. NU_TJ + 1
    for (int n = tid; n < (NU_TI + 1) * (NU_TJ + 3); n += NU_THREADS) {
        const int r = n / (NU_TJ + 3), c = n - r * (NU_TJ + 3);
        const int k = (r + NU_HB) * NU_BW + c + NU_HB - 1;
        const double u = U[k];
        const int ks = k + SU[k] * NU_BW;
#if PYRO_FAST
        const double cx = u * P.dtdx;
#else
        const double cx = u * P.dt / P.dx;                       // advective_fluxes.py:64
#endif
        AX[k] = in_buf1(I0 + r, J0 + c - 1) ? state(u, cx, A[nu_b2a(ks)], SX[ks]) : 0.0;
    }
    // a_y: rows -1 .. NU_TI + 1, columns 0 .. NU_TJ
    for (int n = tid; n < (NU_TI + 3) * (NU_TJ + 1); n += NU_THREADS) {
        const int r = n / (NU_TJ + 1), c = n - r * (NU_TJ + 1);
        const int k = (r + NU_HB - 1) * NU_BW + c + NU_HB;
        const double v = V[k];
        const int ks = k + SV[k];
#if PYRO_FAST
        const double cy = v * P.dtdy;
#else
        const double cy = v * P.dt / P.dy;                       // advective_fluxes.py:65
#endif
        AY[k] = in_buf1(I0 + r - 1, J0 + c) ? state(v, cy, A[nu_b2a(ks)], SY[ks]) : 0.0;
    }
    __syncthreads();

    // ---- 4. fluxes (advective_fluxes.py:104-125); the velocity of cell i sits on its lower face
    //   F_x[i,j] = u*(a_x[i,j] - dtdy2*(F_yt[i+sx,j+1] - F_yt[i+sx,j])),  F_yt = v*a_y
    for (int n = tid; n < (NU_TI + 1) * NU_TJ; n += NU_THREADS) {
        const int r = n / NU_TJ, c = n - r * NU_TJ;
        const int k = (r + NU_HB) * NU_BW + c + NU_HB;
        const int ks = k + SU[k] * NU_BW;
        SX[k] = U[k] * (AX[k] - P.dtdy2 * (V[ks + 1] * AY[ks + 1] - V[ks] * AY[ks]));
    }
    //   F_y[i,j] = v*(a_y[i,j] - dtdx2*(F_xt[i+1,j+sy] - F_xt[i,j+sy])),  F_xt = u*a_x
    for (int n = tid; n < NU_TI * (NU_TJ + 1); n += NU_THREADS) {
        const int r = n / (NU_TJ + 1), c = n - r * (NU_TJ + 1);
        const int k = (r + NU_HB) * NU_BW + c + NU_HB;
        const int ks = k + SV[k];
        SY[k] = V[k] * (AY[k] - P.dtdx2 * (U[ks + NU_BW] * AX[ks + NU_BW] - U[ks] * AX[ks]));
    }
    __syncthreads();

    // ---- 5. update (simulation.py:107-108); ghost cells: the filled value of the old level
    for (int n = tid; n < NU_TI * NU_TJ; n += NU_THREADS) {
        const int r = n / NU_TJ, c = n - r * NU_TJ;
        const int i = I0 + r, j = J0 + c;
        if (i >= g.qx || j >= g.qy) continue;
        const int k = (r + NU_HB) * NU_BW + c + NU_HB;
        double a = A[(r + NU_HA) * NU_AW + c + NU_HA];
        if (i >= g.ilo && i <= g.ihi && j >= g.jlo && j <= g.jhi)
            a = a + P.dtdx * (SX[k] - SX[k + NU_BW]) + P.dtdy * (SY[k] - SY[k + 1]);
        aout[(size_t)i * g.pitch + j] = a;
        if (dump) {     // pyrohip_advnu_stage_dump: a_x, a_y, F_x, F_y of the cell's lower faces
            double *d = dump + (size_t)i * g.pitch + j;
            d[0] = AX[k]; d[g.plane] = AY[k]; d[2 * g.plane] = SX[k]; d[3 * g.plane] = SY[k];
        }
    }
}

// one step from plane `cur` into plane `nxt` (both laid out like a plane of the state)
int advnu_step_launch(pyrohip_state *s, int ia, int iu, int iv, const pyrohip_advnu_params *ap, double dt,
                      const double *cur, double *nxt, double *dump)
{
    pyrohip_ctx *c = s->ctx;
    const Geom &g = s->g;
    AdvNuParams P;
    P.dt = dt; P.dx = ap->dx; P.dy = ap->dy;
    P.dtdx = dt / ap->dx; P.dtdy = dt / ap->dy;
    P.dtdx2 = 0.5 * dt / ap->dx; P.dtdy2 = 0.5 * dt / ap->dy;
    P.gx = (g.qy + NU_TJ - 1) / NU_TJ; P.gy = (g.qx + NU_TI - 1) / NU_TI;
    const int var[3] = {ia, iu, iv};
    for (int m = 0; m < 3; m++)
        for (int k = 0; k < 4; k++) P.bc[4 * m + k] = s->bc[var[m] * 4 + k];
    const double *u = s->d + (size_t)iu * g.plane, *v = s->d + (size_t)iv * g.plane;
    const dim3 grid(xcd_grid_1d(P.gx, P.gy)), block(NU_THREADS);
    if (ap->limiter == 0) PYRO_LAUNCH(c, "k_advnu_step", (k_advnu_step<0>), grid, block, 0, cur, u, v, nxt, g, P,
                    dump);
    else if (ap->limiter == 1) PYRO_LAUNCH(c, "k_advnu_step", (k_advnu_step<1>), grid, block, 0, cur, u, v, nxt, g, P,
                    dump);
    else PYRO_LAUNCH(c, "k_advnu_step", (k_advnu_step<2>), grid, block, 0, cur, u, v, nxt, g, P,
                    dump);
    PYRO_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PYRO_NS
}  // namespace pyro

#if !PYRO_FAST
// ---- extern "C" entry points (in the bit-faithful unit; the contracted unit only adds its
// kernel instances) ----------------------------------------------------------------------
namespace pyro {
namespace fastm {
int advnu_step_launch(pyrohip_state *, int, int, int, const pyrohip_advnu_params *, double, const double *,
                      double *, double *);
}
}  // namespace pyro

using namespace pyro;

static int advnu_check(pyrohip_state *s, int ia, int iu, int iv, const pyrohip_advnu_params *ap)
{
    PYRO_REQUIRE(s && ap, "NULL argument");
    PYRO_REQUIRE(ia >= 0 && ia < s->nvar && iu >= 0 && iu < s->nvar && iv >= 0 && iv < s->nvar,
                 "variable index out of range");
    PYRO_REQUIRE(ia != iu && ia != iv, "the advected variable must not be one of the velocities");
    PYRO_REQUIRE(s->g.ng == 4, "advection_nonuniform is built for ng = 4 (advection_nonuniform/simulation.py:28)");
    PYRO_REQUIRE(s->g.nx >= 4 && s->g.ny >= 4, "the grid must be at least as wide as its ghost frame");
    PYRO_REQUIRE(ap->limiter >= 0 && ap->limiter <= 2, "limiter must be 0, 1 or 2");
    PYRO_REQUIRE(ap->dx > 0.0 && ap->dy > 0.0, "bad dx / dy");
    PYRO_REQUIRE(!s->nb_set, "advection_nonuniform does not step slabs of a decomposed grid");
    const int var[3] = {ia, iu, iv};
    for (int m = 0; m < 3; m++)
        for (int k = 0; k < 4; k++)
            PYRO_REQUIRE(bc_is_index_map(s->bc[var[m] * 4 + k], true),
                         "fused ghost fill: outflow / reflect / periodic boundaries only");
    return 0;
}

// nsteps x (ghost fill of the density, u and v + step), alternating between the density's plane
// of the state and the work plane (common.h: evolve_pingpong)
extern "C" int pyrohip_advnu_evolve(pyrohip_state *s, int ia, int iu, int iv, const pyrohip_advnu_params *ap,
                                    const double *dts, int nsteps)
{
    PYRO_TRY(advnu_check(s, ia, iu, iv, ap));
    PYRO_REQUIRE(dts || nsteps == 0, "NULL argument");
    PYRO_REQUIRE(nsteps >= 0, "negative step count");
    auto step = [&](int k, const double *cur, double *nxt) {
        return PYRO_BUILD(ap->fast_math, advnu_step_launch(s, ia, iu, iv, ap, dts[k], cur, nxt, nullptr));
    };
    return evolve_pingpong(s, ia, WorkOwner::ADVNU, 1, nsteps, step);
}

extern "C" int pyrohip_advnu_step(pyrohip_state *s, int ia, int iu, int iv, const pyrohip_advnu_params *ap,
                                  double dt)
{
    return pyrohip_advnu_evolve(s, ia, iu, iv, ap, &dt, 1);
}

// test hook: the intermediates of one step from the state as it is -- a_x, a_y, F_x, F_y on the
// lower faces of every cell, four (qx, qy) host arrays one after the other.  The state is not
// changed (the new level goes to the work plane and is dropped).  Meaningful where the update
// reads them: rows ilo .. ihi + 1, columns jlo .. jhi + 1.
extern "C" int pyrohip_advnu_stage_dump(pyrohip_state *s, int ia, int iu, int iv,
                                        const pyrohip_advnu_params *ap, double dt, double *host)
{
    PYRO_TRY(advnu_check(s, ia, iu, iv, ap));
    PYRO_REQUIRE(host, "NULL argument");
    const Geom &g = s->g;
    PYRO_TRY(comm_wait_halo(s));
    PYRO_TRY(state_work(s, WorkOwner::ADVNU, 1));
    DevBuf tmp;
    PYRO_TRY(tmp.ensure(4 * g.plane * sizeof(double)));
    double *dump = (double *)tmp.p;
    const int rc = PYRO_BUILD(ap->fast_math, advnu_step_launch(s, ia, iu, iv, ap, dt, s->d + (size_t)ia * g.plane,
                                                               s->work + geom_lead(g), dump));
    return dump_planes_to_host(s, tmp, 4, rc, hipSuccess, host);
}

// method_compute_timestep (advection_nonuniform/simulation.py:64-82): the maxima run over the
// whole array, ghost cells AS THEY ARE IN MEMORY included (the driver fills them first); no floor
// on the velocity -- a zero maximum gives inf and the other direction decides
extern "C" int pyrohip_advnu_dt(pyrohip_state *s, int iu, int iv, double dx, double dy, double cfl, double *dt)
{
    PYRO_REQUIRE(s && dt, "NULL argument");
    PYRO_REQUIRE(dx > 0.0 && dy > 0.0, "bad dx / dy");
    double lo, hi;
    PYRO_TRY(pyrohip_state_minmax(s, iu, s->g.ng, &lo, &hi));
    const double umax = fabs(lo) > fabs(hi) ? fabs(lo) : fabs(hi);
    PYRO_TRY(pyrohip_state_minmax(s, iv, s->g.ng, &lo, &hi));
    const double vmax = fabs(lo) > fabs(hi) ? fabs(lo) : fabs(hi);
    const double xtmp = dx / umax, ytmp = dy / vmax;
    *dt = cfl * (ytmp < xtmp ? ytmp : xtmp);
    return 0;
}
#endif
