// Method-of-lines advection of a scalar with a constant velocity (advection_rk: second order,
// advection_fv4: fourth order, advection_weno: WENO reconstructions of Lax-Friedrichs split
// fluxes): ONE launch per Runge-Kutta stage.
//
// Replaces (reference file:line)
//   pyro/advection_rk/simulation.py:10-90        substep, evolve
//   pyro/advection_rk/fluxes.py:52-100           fluxes (second order)
//   pyro/advection_fv4/fluxes.py:52-116          fluxes (fourth order)
//   pyro/advection_weno/fluxes.py:6-105          fvs, fluxes (WENO)
//   pyro/mesh/reconstruction.py:186-258          weno_upwind and its constants
//   pyro/mesh/fourth_order.py:8-235              states (fv4_limit.h: mc_limit)
//   pyro/mesh/reconstruction.py:9-120            limit / limit2 / limit4 (stencil.h)
//   pyro/mesh/integration.py:103-129             get_stage_start, compute_final_update
//   pyro/mesh/array_indexer.py:150-274           fill_ghost of every stage start
//
// k_advrk_stage<SCHEME, NK, LAST> works on 2-d tiles in LDS and does, in one launch, what the
// stage-by-stage path does in three (pyrohip_state_lincomb, ghost fill, right-hand side):
//   1. the stage start y_s = y_n + c_0 k_0 + ... + c_{NK-1} k_{NK-1} is formed AS THE TILE IS
//      LOADED, every cell from its interior source cell under the boundary rules (the reference
//      clones, adds on the interior, then fills: a ghost cell of the stage start is the stage
//      value of its source cell).  The products and the order of accumulation are k_lincomb's;
//      every coefficient is applied, zeros included.  No stage-start plane exists in memory.
//   2. face values, fluxes and k_s = -div F of the tile (second order: limited slopes, upwind
//      face value, F = u a; fourth order: face averages -- Eq. 17 or the limited states --,
//      face centres by the transverse Laplacian, F = u a_cc + lap_t(u a) / 24; WENO: per face
//      the two reconstructions of (u a +- alpha a) / 2 from the 2 R cells around it).
//   3. LAST: the final update y_{n+1} = y_n + sum b_s dt k_s (compute_final_update's order, the
//      stage's own k_s from registers) into a SECOND plane -- neighbouring tiles still read y_n
//      for their halos in this launch; ghost cells of the new plane get the filled value of
//      y_n, which is what the reference leaves there (its stage 0 fills y_n in place, the final
//      update touches the interior only).  The last k_s is not written to memory.
//
// Halo (derived from the reference's loop ranges; the update reads F_x on rows ilo .. ihi + 1,
// F_y on columns jlo .. jhi + 1):
//   second order: the face's upwind cell is one of the two beside it, its limit4 slope reads a at
//                 +-2 through the limit2 of its neighbours: 3 cells; no transverse reach.
//   fourth order: the limited state of a face comes from the cell behind it (u > 0) or in front of
//                 it, whose limiter reads a at +-3 (d3a at +2 reads d2ac at +2): 4 cells in the
//                 sweep direction; the transverse Laplacians reach one face sideways: 1 cell.
//                 The tile keeps ONE array of a with the larger apron on all four sides (the x
//                 sweep needs rows +-4 x columns +-1, the y sweep the transpose).
//   WENO:         face i reads cells i - R .. i + R - 1 (R = weno_order, 2 or 3): the second-order
//                 tile with its 3 cells; no transverse reach.  ng = 4 > R: none of the zeros at
//                 the ends of the reference's flux_p_r / flux_m_l reaches a face the update reads.
// Nothing of the reference's zero-initialised scratch arrays is read inside those ranges except
// d3a above the y sweep's last cell (mc_limit's d3a_top_zero), which is repeated.
//
// LDS (TI = 16, TJ = 32, 256 threads; y, the contiguous index, runs across the lanes, so that
// neighbouring lanes read neighbouring 8-byte words -- conflict-free -- whichever neighbour of a
// cell the stencil takes):      second order and WENO 14.9 KiB (+4 KiB in the last stage): 8
// workgroups per CU; fourth order 25.0 KiB (+4 KiB): 5 workgroups = 20 wavefronts per CU.
//
// Compiled twice (build.py): bit-faithful (-ffp-contract=off, true divisions by dx, dy) and
// contracted (-ffp-contract=fast, reciprocals); pyrohip_advrk_params.fast_math selects.
// Two places of weno_upwind are not plain IEEE operations in the reference: np.dot at its end is
// a chain of fused multiply-adds in the reference's BLAS -- the bit-faithful unit calls fma()
// there --, and beta**2 is the C library's pow(), which is not always the product (libm_pow2.h).
#include <cmath>

#include "builds.h"
#include "common.h"
#include "stencil.h"
#include "fv4_limit.h"
#include "libm_pow2.h"

namespace pyro {

constexpr int RK_TI = 16, RK_TJ = 32, RK_THREADS = 256;
constexpr int RK_DUMP_PLANES = 6;

struct AdvRkArgs {
    double dx, dy, rdx, rdy, u, v;
    double alpha;       // WENO: the speed of the Lax-Friedrichs split, sqrt(u^2 + v^2)
    double ca[3];       // dt a[s][0 .. NK): the stage start
    double cb[4];       // dt b[0 .. NK]: the final update (LAST)
    int limiter;
    int gx, gy;         // tiles across (columns) / down (rows)
    int oj;             // columns of the first tile column that lie in front of the array
    int bc[4];          // xl, xr, yl, yr of the variable
};

namespace PYRO_NS {

// mesh/reconstruction.py:224-258: weno_upwind of the window p[0 .. 2 R - 2], the reference's
// operations in its order (beta and the stencil values start at 0.0; sigma's entries with m > l
// are not visited).  The constants are the quotients the reference forms (:188-212).
template <int R>
__device__ __forceinline__ double weno_upwind(const double *p)
{
    static_assert(R == 2 || R == 3, "weno_order 2 or 3");
    const double C3[3] = {1. / 10., 6. / 10., 3. / 10.};
    const double a3[3][3] = {{11. / 6., -7. / 6., 2. / 6.}, {2. / 6., 5. / 6., -1. / 6.}, {-1. / 6., 5. / 6., 2. / 6.}};
    const double s3[3][3][3] = {{{40. / 12., 0, 0}, {-124. / 12., 100. / 12., 0}, {44. / 12., -76. / 12., 16. / 12.}},
                                {{16. / 12., 0, 0}, {-52. / 12., 52. / 12., 0}, {20. / 12., -52. / 12., 16. / 12.}},
                                {{16. / 12., 0, 0}, {-76. / 12., 100. / 12., 0}, {44. / 12., -124. / 12., 40. / 12.}}};
    const double C2[3] = {1. / 3., 2. / 3., 0};
    const double a2[3][3] = {{3. / 2., -1. / 2., 0}, {1. / 2., 1. / 2., 0}, {0, 0, 0}};
    const double s2[3][3][3] = {{{1., 0, 0}, {-2., 1., 0}, {0, 0, 0}}, {{1., 0, 0}, {-2., 1., 0}, {0, 0, 0}},
                                {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}};
    double al[R], st[R];
#pragma unroll
    for (int k = 0; k < R; k++) {
        double beta = 0.0, sk = 0.0;
#pragma unroll
        for (int l = 0; l < R; l++) {
#pragma unroll
            for (int m = 0; m <= l; m++)
                beta += ((R == 3 ? s3[k][l][m] : s2[k][l][m]) * p[R - 1 + k - l]) * p[R - 1 + k - m];
        }
#if PYRO_FAST
        const double b2 = beta * beta;
#else
        const double b2 = square_as_libm_pow(beta);      // beta[k]**2 is the C library's pow()
#endif
        al[k] = (R == 3 ? C3[k] : C2[k]) / (1e-16 + b2);
#pragma unroll
        for (int l = 0; l < R; l++) sk += (R == 3 ? a3[k][l] : a2[k][l]) * p[R - 1 + k - l];
        st[k] = sk;
    }
    double sum = al[0] + al[1];
    if constexpr (R == 3) sum += al[2];
#if PYRO_FAST
    double d = al[0] * st[0] + al[1] * st[1];
    if constexpr (R == 3) d += al[2] * st[2];
    return d * (1.0 / sum);
#else
    // np.dot(w, q_stencils): fused multiply-adds from 0, in order
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < R; k++) d = fma(al[k] / sum, st[k], d);
    return d;
#endif
}

template <int SCHEME>
struct RkTile {
    static constexpr int H = SCHEME == 4 ? 4 : 3;          // apron of a
    static constexpr int T = SCHEME == 4 ? 1 : 0;          // transverse reach of the face values
    static constexpr int AH = RK_TI + 2 * H, AW = RK_TJ + 2 * H;
    static constexpr int XW = RK_TJ + 2 * T, NX = (RK_TI + 1) * XW;          // x faces 0 .. TI
    static constexpr int YW = RK_TJ + 1, NY = (RK_TI + 2 * T) * YW;          // y faces 0 .. TJ
    static constexpr int NFX = SCHEME == 4 ? (RK_TI + 1) * RK_TJ : 1;
    static constexpr int NFY = SCHEME == 4 ? RK_TI * (RK_TJ + 1) : 1;
};

// SCHEME 2 | 4 | 5 (WENO; R = weno_order, 0 otherwise)
template <int SCHEME, int NK, bool LAST, int R = 0>
__global__ __launch_bounds__(RK_THREADS) void k_advrk_stage(const double *__restrict__ y,
                                                            const double *__restrict__ kin, size_t kstride,
                                                            double *__restrict__ kout,
                                                            double *__restrict__ ynew, Geom g, AdvRkArgs P,
                                                            double *__restrict__ dump)
{
    using TL = RkTile<SCHEME>;
    constexpr int H = TL::H, T = TL::T, AW = TL::AW, TI = RK_TI, TJ = RK_TJ;
    __shared__ double A[TL::AH * TL::AW];      // the stage start
    __shared__ double QX[TL::NX], QY[TL::NY];  // second order, WENO: F_x, F_y; fourth order: face averages
    __shared__ double FX[TL::NFX], FY[TL::NFY];
    __shared__ double Y1[LAST ? TI * TJ : 1];  // y_n + sum_{s < NK} b_s dt k_s (ghost cells: filled y_n)
    int bx, by;
    if (!xcd_block_2d(P.gx, P.gy, bx, by)) return;
    const int I0 = by * TI, J0 = bx * TJ - P.oj;   // first array cell of the tile (J0 may be < 0)
    const int tid = threadIdx.x;
    const double u = P.u, v = P.v;
    const BcMap mr = bc_map(g.ilo, g.ihi, g.ng, P.bc[0], P.bc[1], true);
    const BcMap mc = bc_map(g.jlo, g.jhi, g.ng, P.bc[2], P.bc[3], true);
    auto in_array = [&](int i, int j) { return i < g.qx && j >= 0 && j < g.qy; };

    // ---- 1. the stage start, through the ghost fill
    for (int n = tid; n < TL::AH * AW; n += RK_THREADS) {
        const int r = n / AW, c = n - r * AW;
        const size_t o = tile_src_off(g, mr, mc, I0 + r - H, J0 + c - H);
        double a = y[o];
#pragma unroll
        for (int s = 0; s < NK; s++) a += P.ca[s] * kin[s * kstride + o];
        A[n] = a;
    }
    if constexpr (LAST) {
        for (int n = tid; n < TI * TJ; n += RK_THREADS) {
            const int r = n / TJ, c = n - r * TJ;
            const int i = I0 + r, j = J0 + c;
            const size_t o = tile_src_off(g, mr, mc, i, j);
            double a = y[o];
            if (i >= g.ilo && i <= g.ihi && j >= g.jlo && j <= g.jhi) {
#pragma unroll
                for (int s = 0; s < NK; s++) a += P.cb[s] * kin[s * kstride + o];
            }
            Y1[n] = a;
        }
    }
    __syncthreads();

    // ---- 2. face values on the lower faces
    if constexpr (SCHEME == 2) {
        // advection_rk/fluxes.py:62-98: the upwind cell's value and limited slope; u == 0 takes
        // the cell behind the face
        auto slope = [&](double am2, double am1, double a0, double ap1, double ap2) {
            if (P.limiter == 0) return 0.5 * (ap1 - am1);
            if (P.limiter == 1) return limit2(am1, a0, ap1);
            return limit4_from(limit2(am2, am1, a0), limit2(a0, ap1, ap2), am1, a0, ap1);
        };
        for (int n = tid; n < (TI + 1) * TJ; n += RK_THREADS) {
            const int r = n / TJ, c = n - r * TJ;
            const bool neg = u < 0.0;
            const int k = ((neg ? r : r - 1) + H) * AW + c + H;
            const double sl = slope(A[k - 2 * AW], A[k - AW], A[k], A[k + AW], A[k + 2 * AW]);
            const double ax = neg ? A[k] - 0.5 * sl : A[k] + 0.5 * sl;
            const double f = u * ax;
            QX[n] = f;
            if (dump && r < TI && in_array(I0 + r, J0 + c)) {
                double *d = dump + (size_t)(I0 + r) * g.pitch + J0 + c;
                d[0] = ax; d[2 * g.plane] = f;
            }
        }
        for (int n = tid; n < TI * (TJ + 1); n += RK_THREADS) {
            const int r = n / (TJ + 1), c = n - r * (TJ + 1);
            const bool neg = v < 0.0;
            const int k = (r + H) * AW + (neg ? c : c - 1) + H;
            const double sl = slope(A[k - 2], A[k - 1], A[k], A[k + 1], A[k + 2]);
            const double ay = neg ? A[k] - 0.5 * sl : A[k] + 0.5 * sl;
            const double f = v * ay;
            QY[n] = f;
            if (dump && c < TJ && in_array(I0 + r, J0 + c)) {
                double *d = dump + (size_t)(I0 + r) * g.pitch + J0 + c;
                d[g.plane] = ay; d[3 * g.plane] = f;
            }
        }
        __syncthreads();
    } else if constexpr (SCHEME == 5) {
        // advection_weno/fluxes.py:28-39, 96-103: F = weno_upwind(f+ behind the face, left to
        // right) + weno_upwind(f- in front of it, right to left), f+- = (vel a +- alpha a) / 2.
        // x and y faces in ONE loop with one body -- the face's first cell and the stride along
        // its pencil differ, nothing else --: 1072 faces are 5 passes of the workgroup, not 3 + 3,
        // and the wavefront that holds the last x and the first y faces does not run the body twice
        constexpr int NFX = (TI + 1) * TJ, NF = NFX + TI * (TJ + 1);
#if PYRO_FAST
        const double cpx = 0.5 * (u + P.alpha), cmx = 0.5 * (u - P.alpha);
        const double cpy = 0.5 * (v + P.alpha), cmy = 0.5 * (v - P.alpha);
#endif
        for (int n = tid; n < NF; n += RK_THREADS) {
            const bool isx = n < NFX;
            const int m = isx ? n : n - NFX, w = isx ? TJ : TJ + 1;
            const int r = m / w, c = m - r * w;
            const int k = (r + H) * AW + c + H, sd = isx ? AW : 1;      // the cell in front of the face
            double fp[2 * R], fm[2 * R];
#pragma unroll
            for (int e = 0; e < 2 * R; e++) {
                const double q = A[k + (e - R) * sd];
#if PYRO_FAST
                fp[e] = (isx ? cpx : cpy) * q;
                fm[2 * R - 1 - e] = (isx ? cmx : cmy) * q;
#else
                const double fl = (isx ? u : v) * q, aq = P.alpha * q;
                fp[e] = (fl + aq) / 2;
                fm[2 * R - 1 - e] = (fl - aq) / 2;
#endif
            }
            const double fpr = weno_upwind<R>(fp), f = fpr + weno_upwind<R>(fm);
            (isx ? QX : QY)[m] = f;
            if (dump && (isx ? r < TI : c < TJ) && in_array(I0 + r, J0 + c)) {
                double *d = dump + (isx ? 0 : g.plane) + (size_t)(I0 + r) * g.pitch + J0 + c;
                d[0] = fpr; d[2 * g.plane] = f;
            }
        }
        __syncthreads();
    } else {
        // advection_fv4/fluxes.py:64-84: face averages.  Limited: a_l (from the cell behind the
        // face) when the velocity is > 0, else a_r (from the cell in front of it) -- u == 0
        // takes a_r, the other way round from the second-order scheme
        for (int n = tid; n < TL::NX; n += RK_THREADS) {
            const int f = n / TL::XW, b = n - f * TL::XW - T;
            const int k = (f + H) * AW + b + H;
            double ax;
            if (P.limiter == 0) {
                ax = 7. / 12. * (A[k - AW] + A[k]) - 1. / 12. * (A[k - 2 * AW] + A[k + AW]);
            } else {
                const bool pos = u > 0.0;
                const int kc = pos ? k - AW : k;
                double w[7], ar, al1;
#pragma unroll
                for (int m = 0; m < 7; m++) w[m] = A[kc + (m - 3) * AW];
                mc_limit(w, false, ar, al1);
                ax = pos ? al1 : ar;
            }
            QX[n] = ax;
            if (dump && f < TI && b >= 0 && b < TJ && in_array(I0 + f, J0 + b))
                dump[(size_t)(I0 + f) * g.pitch + J0 + b] = ax;
        }
        for (int n = tid; n < TL::NY; n += RK_THREADS) {
            const int a = n / TL::YW - T, f = n - (a + T) * TL::YW;
            const int k = (a + H) * AW + f + H;
            double ay;
            if (P.limiter == 0) {
                ay = 7. / 12. * (A[k - 1] + A[k]) - 1. / 12. * (A[k - 2] + A[k + 1]);
            } else {
                const bool pos = v > 0.0;
                const int kc = pos ? k - 1 : k;
                double w[7], ar, al1;
#pragma unroll
                for (int m = 0; m < 7; m++) w[m] = A[kc + (m - 3)];
                // (fourth_order.py:176-179: d3a above the y sweep's last cell is never filled)
                mc_limit(w, J0 + (pos ? f - 1 : f) == g.jhi + 1, ar, al1);
                ay = pos ? al1 : ar;
            }
            QY[n] = ay;
            if (dump && a >= 0 && a < TI && f < TJ && in_array(I0 + a, J0 + f))
                dump[g.plane + (size_t)(I0 + a) * g.pitch + J0 + f] = ay;
        }
        __syncthreads();
        // face centres by the transverse Laplacian, F = u a_cc + lap_t(u a) / 24 (fluxes.py:86-114)
        const double c24 = 1. / 24;
        for (int n = tid; n < (TI + 1) * TJ; n += RK_THREADS) {
            const int f = n / TJ, b = n - f * TJ;
            const double qm = QX[f * TL::XW + b], q0 = QX[f * TL::XW + b + 1], qp = QX[f * TL::XW + b + 2];
            const double acc = q0 - c24 * (qm - 2 * q0 + qp);
            const double F = u * acc + c24 * (u * qm - 2 * (u * q0) + u * qp);
            FX[n] = F;
            if (dump && f < TI && in_array(I0 + f, J0 + b))
                dump[2 * g.plane + (size_t)(I0 + f) * g.pitch + J0 + b] = F;
        }
        for (int n = tid; n < TI * (TJ + 1); n += RK_THREADS) {
            const int a = n / (TJ + 1), f = n - a * (TJ + 1);
            const double qm = QY[a * TL::YW + f], q0 = QY[(a + 1) * TL::YW + f], qp = QY[(a + 2) * TL::YW + f];
            const double acc = q0 - c24 * (qm - 2 * q0 + qp);
            const double F = v * acc + c24 * (v * qm - 2 * (v * q0) + v * qp);
            FY[n] = F;
            if (dump && f < TJ && in_array(I0 + a, J0 + f))
                dump[3 * g.plane + (size_t)(I0 + a) * g.pitch + J0 + f] = F;
        }
        __syncthreads();
    }

    // ---- 3. k_s = -div F on the interior; LAST: the new level on the whole array
    const double *Fx = SCHEME == 4 ? FX : QX, *Fy = SCHEME == 4 ? FY : QY;
    for (int n = tid; n < TI * TJ; n += RK_THREADS) {
        const int r = n / TJ, c = n - r * TJ;
        const int i = I0 + r, j = J0 + c;
        if (!in_array(i, j)) continue;
        const size_t o = (size_t)i * g.pitch + j;
        const bool interior = i >= g.ilo && i <= g.ihi && j >= g.jlo && j <= g.jhi;
        double k = 0.0;
        if (interior) {
            const double ddx = Fx[r * TJ + c] - Fx[(r + 1) * TJ + c];
            const double ddy = Fy[r * (TJ + 1) + c] - Fy[r * (TJ + 1) + c + 1];
#if PYRO_FAST
            k = ddx * P.rdx + ddy * P.rdy;
#else
            k = ddx / P.dx + ddy / P.dy;                 // advection_rk/simulation.py:25-27
#endif
            if constexpr (!LAST) kout[o] = k;
        }
        if constexpr (LAST) ynew[o] = interior ? Y1[n] + P.cb[NK] * k : Y1[n];
        if (dump) {
            dump[4 * g.plane + o] = k;
            dump[5 * g.plane + o] = A[(r + H) * AW + c + H];
        }
    }
}

// one stage: reads plane y and the increments kin[0 .. nk), writes kout (not LAST) or ynew (LAST)
int advrk_stage_launch(pyrohip_state *s, int var, const pyrohip_advrk_params *ap, const double *y,
                       const double *kin, size_t kstride, int nk, bool last, const double *ca,
                       const double *cb, double *kout, double *ynew, double *dump)
{
    pyrohip_ctx *c = s->ctx;
    const Geom &g = s->g;
    AdvRkArgs P;
    P.dx = ap->dx; P.dy = ap->dy; P.rdx = 1.0 / ap->dx; P.rdy = 1.0 / ap->dy;
    P.u = ap->u; P.v = ap->v; P.alpha = ap->scheme == 5 ? ap->alpha : 0.0;
    for (int k = 0; k < 3; k++) P.ca[k] = ca ? ca[k] : 0.0;
    for (int k = 0; k < 4; k++) P.cb[k] = cb ? cb[k] : 0.0;
    P.limiter = ap->limiter;
    P.oj = RK_TJ - g.ng;           // the interior starts on a tile boundary: aligned rows
    P.gx = (g.qy + P.oj + RK_TJ - 1) / RK_TJ; P.gy = (g.qx + RK_TI - 1) / RK_TI;
    for (int k = 0; k < 4; k++) P.bc[k] = s->bc[var * 4 + k];
    const dim3 grid(xcd_grid_1d(P.gx, P.gy)), block(RK_THREADS);
#define ADVRK_GO(SCH, NK, LAST, R)                                                                    \
    PYRO_LAUNCH(c, "k_advrk_stage", (k_advrk_stage<SCH, NK, LAST, R>), grid, block, 0, y, kin,        \
                kstride, kout, ynew, g, P, dump)
#define ADVRK_SCHEME(SCH, R)                                                                          \
    do {                                                                                              \
        if (!last) {                                                                                  \
            if (nk == 0) ADVRK_GO(SCH, 0, false, R);                                                  \
            else if (nk == 1) ADVRK_GO(SCH, 1, false, R);                                             \
            else ADVRK_GO(SCH, 2, false, R);                                                          \
        } else {                                                                                      \
            if (nk == 1) ADVRK_GO(SCH, 1, true, R);                                                   \
            else if (nk == 2) ADVRK_GO(SCH, 2, true, R);                                              \
            else ADVRK_GO(SCH, 3, true, R);                                                           \
        }                                                                                             \
    } while (0)
    if (ap->scheme == 2) ADVRK_SCHEME(2, 0);
    else if (ap->scheme == 4) ADVRK_SCHEME(4, 0);
    else if (ap->weno_order == 2) ADVRK_SCHEME(5, 2);
    else ADVRK_SCHEME(5, 3);
#undef ADVRK_SCHEME
#undef ADVRK_GO
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
int advrk_stage_launch(pyrohip_state *, int, const pyrohip_advrk_params *, const double *, const double *,
                       size_t, int, bool, const double *, const double *, double *, double *, double *);
}
}  // namespace pyro

using namespace pyro;

namespace {

// Butcher tableaux of mesh/integration.py:32-70
struct Tableau { int ns; double a[4][4]; double b[4]; };
const Tableau kTableau[4] = {
    {2, {{0.0, 0.0}, {0.5, 0.0}}, {0.0, 1.0}},                                           // RK2
    {2, {{0.0, 0.0}, {1.0, 0.0}}, {0.5, 0.5}},                                           // TVD2
    {3, {{0.0, 0.0, 0.0}, {1.0, 0.0, 0.0}, {0.25, 0.25, 0.0}}, {1. / 6., 1. / 6., 2. / 3.}},   // TVD3
    {4, {{0.0, 0.0, 0.0, 0.0}, {0.5, 0.0, 0.0, 0.0}, {0.0, 0.5, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}},
     {1. / 6., 1. / 3., 1. / 3., 1. / 6.}},                                              // RK4
};

int advrk_check(pyrohip_state *s, int var, const pyrohip_advrk_params *ap)
{
    PYRO_REQUIRE(s && ap, "NULL argument");
    PYRO_REQUIRE(var >= 0 && var < s->nvar, "variable index out of range");
    PYRO_REQUIRE(s->g.ng == 4, "advection_rk / advection_fv4 / advection_weno are built for ng = 4");
    PYRO_REQUIRE(s->g.nx >= 4 && s->g.ny >= 4, "the grid must be at least as wide as its ghost frame");
    PYRO_REQUIRE(ap->scheme == 2 || ap->scheme == 4 || ap->scheme == 5,
                 "scheme must be 2 (advection_rk), 4 (advection_fv4) or 5 (advection_weno)");
    if (ap->scheme == 5) {
        // (advection_weno/fluxes.py:89: the reference's assert)
        PYRO_REQUIRE(ap->weno_order == 2 || ap->weno_order == 3, "advection_weno: weno_order must be 2 or 3");
        PYRO_REQUIRE(ap->alpha >= 0.0 && std::isfinite(ap->alpha),
                     "advection_weno: alpha must be finite and not negative");
    }
    PYRO_REQUIRE(ap->limiter >= 0, "negative limiter");
    PYRO_REQUIRE(ap->scheme != 2 || ap->limiter < 10,
                 "advection_rk: limiter >= 10 does not run in the reference (advection_rk/fluxes.py:72)");
    PYRO_REQUIRE(ap->dx > 0.0 && ap->dy > 0.0, "bad dx / dy");
    PYRO_REQUIRE(!s->nb_set, "advection_rk / advection_fv4 do not step slabs of a decomposed grid");
    for (int k = 0; k < 4; k++)
        PYRO_REQUIRE(bc_is_index_map(s->bc[var * 4 + k], false),
                     "fused ghost fill: outflow / reflect-even / periodic boundaries only");
    return 0;
}

// work planes: the other level of the ping-pong, then the increments of all stages but the last
constexpr size_t kAdvRkWork = 4;

// the stages 0 .. upto of one step from plane cur; the last stage writes plane nxt.  dump: the
// intermediates of stage `upto` (pyrohip_advrk_stage_dump)
int advrk_stages(pyrohip_state *s, int var, const pyrohip_advrk_params *ap, const Tableau &tb, double dt,
                 const double *cur, double *nxt, int upto, double *dump)
{
    const Geom &g = s->g;
    double *kpl = s->work + geom_lead(g) + g.plane;
    for (int st = 0; st <= upto; st++) {
        const bool last = st == tb.ns - 1;
        double ca[3] = {0, 0, 0}, cb[4] = {0, 0, 0, 0};
        for (int k = 0; k < st; k++) ca[k] = dt * tb.a[st][k];              // integration.py:111
        if (last)
            for (int k = 0; k < tb.ns; k++) cb[k] = dt * tb.b[k];           // integration.py:125
        double *kout = last ? nullptr : kpl + (size_t)st * g.plane;
        double *d = st == upto ? dump : nullptr;
        PYRO_TRY(PYRO_BUILD(ap->fast_math,
                            advrk_stage_launch(s, var, ap, cur, kpl, g.plane, st, last, ca, cb, kout, nxt, d)));
    }
    return 0;
}

}  // namespace

extern "C" int pyrohip_advrk_rhs(pyrohip_state *y, int var, const pyrohip_advrk_params *ap,
                                 pyrohip_state *kstate, int slot)
{
    PYRO_TRY(advrk_check(y, var, ap));
    PYRO_REQUIRE(kstate, "NULL argument");
    PYRO_REQUIRE(slot >= 0 && slot < kstate->nvar, "slot out of range");
    PYRO_REQUIRE(kstate != y, "the increments need a state of their own");
    PYRO_REQUIRE(kstate->ctx == y->ctx, "states live on different contexts");
    PYRO_REQUIRE(kstate->g.plane == y->g.plane && kstate->g.nx == y->g.nx && kstate->g.ny == y->g.ny &&
                     kstate->g.ng == y->g.ng,
                 "geometries differ");
    PYRO_TRY(comm_wait_halo(y));
    const double *cur = y->d + (size_t)var * y->g.plane;
    double *kout = kstate->d + (size_t)slot * y->g.plane;
    return PYRO_BUILD(ap->fast_math, advrk_stage_launch(y, var, ap, cur, nullptr, 0, 0, false, nullptr, nullptr,
                                                        kout, nullptr, nullptr));
}

// nsteps Runge-Kutta steps, nstages launches each, alternating between the variable's plane of
// the state and a work plane (common.h: evolve_pingpong)
extern "C" int pyrohip_advrk_evolve(pyrohip_state *s, int var, const pyrohip_advrk_params *ap, int method,
                                    const double *dts, int nsteps)
{
    PYRO_TRY(advrk_check(s, var, ap));
    PYRO_REQUIRE(method >= 0 && method <= 3, "unknown temporal method");
    PYRO_REQUIRE(dts || nsteps == 0, "NULL argument");
    PYRO_REQUIRE(nsteps >= 0, "negative step count");
    const Tableau &tb = kTableau[method];
    auto step = [&](int k, const double *cur, double *nxt) {
        return advrk_stages(s, var, ap, tb, dts[k], cur, nxt, tb.ns - 1, nullptr);
    };
    return evolve_pingpong(s, var, WorkOwner::ADVRK, kAdvRkWork, nsteps, step);
}

extern "C" int pyrohip_advrk_step(pyrohip_state *s, int var, const pyrohip_advrk_params *ap, int method,
                                  double dt)
{
    return pyrohip_advrk_evolve(s, var, ap, method, &dt, 1);
}

// test hook: the intermediates of stage `stage` of one step from the state as it is -- a_x, a_y
// (WENO: the reconstructed positive parts, flux_p_r of fvs, in x and y), F_x, F_y on the lower
// faces of every cell, k_s and the stage start: six (qx, qy) host arrays one after the other.
// The state is not changed.
extern "C" int pyrohip_advrk_stage_dump(pyrohip_state *s, int var, const pyrohip_advrk_params *ap,
                                        int method, double dt, int stage, double *host)
{
    PYRO_TRY(advrk_check(s, var, ap));
    PYRO_REQUIRE(method >= 0 && method <= 3, "unknown temporal method");
    PYRO_REQUIRE(host, "NULL argument");
    const Tableau &tb = kTableau[method];
    PYRO_REQUIRE(stage >= 0 && stage < tb.ns, "stage out of range");
    pyrohip_ctx *c = s->ctx;
    const Geom &g = s->g;
    PYRO_TRY(comm_wait_halo(s));
    PYRO_TRY(state_work(s, WorkOwner::ADVRK, kAdvRkWork));
    DevBuf tmp;
    PYRO_TRY(tmp.ensure(RK_DUMP_PLANES * g.plane * sizeof(double)));
    double *dump = (double *)tmp.p;
    const hipError_t e = hipMemsetAsync(dump, 0, RK_DUMP_PLANES * g.plane * sizeof(double), c->stream);
    int rc = 0;
    if (e == hipSuccess)
        rc = advrk_stages(s, var, ap, tb, dt, s->d + (size_t)var * g.plane, s->work + geom_lead(g), stage, dump);
    return dump_planes_to_host(s, tmp, RK_DUMP_PLANES, rc, e, host);
}

// test hook: square_as_libm_pow (libm_pow2.h) of n host values, as the bit-faithful WENO kernels
// evaluate it
namespace {
__global__ void k_test_square_as_pow(const double *__restrict__ x, size_t n, double *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = square_as_libm_pow(x[i]);
}
}  // namespace

extern "C" int pyrohip_test_square_as_pow(pyrohip_ctx *c, const double *x, size_t n, double *out)
{
    PYRO_REQUIRE(c && (n == 0 || (x && out)), "NULL argument");
    PYRO_REQUIRE(n <= ((size_t)1 << 28), "at most 2^28 values in one call");
    if (n == 0) return 0;
    DevBuf buf;
    PYRO_TRY(buf.ensure(2 * n * sizeof(double)));
    double *dx = (double *)buf.p, *dout = dx + n;
    hipError_t e = hipMemcpyAsync(dx, x, n * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        PYRO_LAUNCH(c, "k_test_square_as_pow", k_test_square_as_pow, dim3((unsigned)((n + 255) / 256)), dim3(256),
                    0, dx, n, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    buf.release();
    PYRO_CHECK_HIP(e);
    PYRO_CHECK_HIP(e2);
    return 0;
}
#endif
