// compressible_rk: one Runge-Kutta stage as ONE launch of a 2-d LDS tile kernel (kernel_set 1, and
// the library's choice below the row-marching kernel's size).
//
// Replaces, per stage (reference file:line)
//   pyro/compressible_rk/simulation.py:10-104   k = -div F + S, the stage loop, the time step
//   pyro/compressible_rk/fluxes.py:28-180       piecewise-linear states, Riemann problems, viscosity
//   pyro/mesh/integration.py:105-129            stage starts and the final update
//
// Same arithmetic as the staged kernels of compressible.hip (k_prim, k_xi, k_rk_states<false>,
// k_rk_flux, k_rk_rhs, k_rk_cfl: the bit-faithful build repeats their expressions), but no
// intermediate reaches memory.  A workgroup of RBI x RBJ threads owns the (RBI-2) x (RBJ-2) cells of
// its tile; thread (ti, tj) is cell (i0-1+ti, j0-1+tj): the tile grown by one cell, the region on
// which face states are needed.  Phases, separated by workgroup barriers:
//   0  stage state (tile + 4-cell apron: the flattening coefficient of a cell of R(1) reads the
//      pressure three cells further out) -> density floor, primitives Q in LDS; the conserved
//      energy and momenta of the thread region beside them
//   1  per cell: flattening coefficient, limited slopes, the four face states (lower ones in
//      registers, upper ones -> LDS), vertex div(U) -> LDS
//   2  one Riemann problem on each of the cell's lower faces + artificial viscosity
//      (barrier: every upper state has been read) -> LDS, over the upper states
//   3  k = -div F + gravity of the tile's cells; stored, or -- last stage -- added into
//      y_0 + dt sum_s b_s k_s, with the CFL quantity of the new state
// LDS: 4 Q planes of 22 x 38 + 8 state / flux planes + div(U) + 3 conserved planes of 512 = 74.1 KiB:
// two workgroups (16 wavefronts) per CU.
//
// The stage state never exists in memory: stage 0 reads the ghost-filled state itself, a later
// stage builds y_s = y_0 + dt sum_j a_sj k_j per cell as it is loaded (the accumulation order of
// RKIntegrator; a zero weight adds nothing and is not read), a ghost cell from the interior cell its
// boundary rule copies from, with the sign of an odd reflection.
//
// Compiled twice like compressible.hip (PYRO_FAST = 0 / 1, builds.h; exports: comp_units.h).
#include "builds.h"
#include "common.h"
#include "hydro.h"
#include "reduce.h"

namespace pyro {
namespace PYRO_NS {
#include "comp_units.h"

constexpr int RBI = 16;                 // threads along i (rows)
constexpr int RBJ = 32;                 // threads along j (fast axis)
constexpr int RNT = RBI * RBJ;          // 512
constexpr int RTI = RBI - 2;            // cells per tile
constexpr int RTJ = RBJ - 2;
constexpr int RQH = RBI + 6;            // Q tile rows (thread region + 3 = tile + 4)
constexpr int RQW = RBJ + 6;
constexpr int RQN = RQH * RQW;
constexpr int RLDS_DOUBLES = 4 * RQN + 8 * RNT + RNT + 3 * RNT;
constexpr size_t RLDS_BYTES = (size_t)RLDS_DOUBLES * sizeof(double);
static_assert(2 * (RLDS_BYTES + 1024) <= 160 * 1024, "two workgroups of the stage kernel per CU");
// waves per SIMD the register allocation must allow: 4 = two 512-thread workgroups per CU
constexpr int RK_MINW = 4;

#include "fused_common.h"

enum { RK_FIRST = 0, RK_MIDDLE = 1, RK_LAST = 2 };

__device__ __forceinline__ Cons rkt_get(const double *b, int t)
{
    return Cons{b[t], b[RNT + t], b[2 * RNT + t], b[3 * RNT + t]};
}
__device__ __forceinline__ void rkt_put(double *b, int t, const Cons &U)
{
    b[t] = U.d; b[RNT + t] = U.E; b[2 * RNT + t] = U.mx; b[3 * RNT + t] = U.my;
}
// the quotients of k_rk_rhs / k_rk_cfl: IEEE divisions there, the reciprocal forms in the contracted build
__device__ __forceinline__ double rkt_div(double a, double b)
{
#if PYRO_FAST
    return pdiv(a, b);
#else
    return a / b;
#endif
}
// F += av (Um - Uc), fluxes.py:162-168
__device__ __forceinline__ void rkt_avisc(Cons &F, double av, const Cons &Um, const Cons &Uc)
{
    F.d += av * (Um.d - Uc.d);
    F.E += av * (Um.E - Uc.E);
    F.mx += av * (Um.mx - Uc.mx);
    F.my += av * (Um.my - Uc.my);
}

// SOLVER: compressible.riemann (0 HLLC, 1 CGF, 2 HLLC_lm).  KIND: RK_FIRST stores k_0 and keeps the
// density floor in the state (clean_state works in place); RK_MIDDLE stores k_s; RK_LAST stores the
// new state into P.rk_out and leaves the workgroup's CFL partial.
// Uin: the state y_0 (ghost cells filled in memory: stage 0 reads them); Kout: the 4 planes of this
// stage's k (unused by the last stage).
template <int SOLVER, int KIND>
__global__ __launch_bounds__(RNT, RK_MINW) void k_rk_tile(const double *__restrict__ Uin,
                                                         double *__restrict__ Kout, Geom g, FP P,
                                                         int *__restrict__ flag,
                                                         double *__restrict__ partial,
                                                         const StepScalars *__restrict__ SC)
{
    HIP_DYNAMIC_SHARED(double, lds)
    __shared__ int skip_s;
    const int tile = xcd_tile(blockIdx.x, P.ntiles);
    const int tj = threadIdx.x, ti = threadIdx.y;
    const int t = ti * RBJ + tj;
    double dt = P.dt;
    if (SC) {   // device-side run: this step's dt lives in device memory
        if (!SC->active) {
            // past tmax / after an invalid state: nothing happens (the host picks the buffer that
            // holds the last state that did advance, evolve_close)
            if (KIND == RK_LAST && t == 0) partial[tile] = INFINITY;
            return;
        }
        dt = SC->dt;
    }
    double *Q = lds;                    // rho u v p: the tile + 4-cell apron
    double *S = Q + 4 * RQN;            // upper face states XP(0..3), YP(4..7) | fluxes Fx, Fy
    double *SY = S + 4 * RNT;
    double *D = S + 8 * RNT;            // vertex div(U)
    double *UC = D + RNT;               // energy, x-momentum, y-momentum of the thread region

    const int i0 = g.ilo + (tile / P.ntj) * RTI;
    const int j0 = g.jlo + (tile % P.ntj) * RTJ;
    const int i = i0 - 1 + ti, j = j0 - 1 + tj;
    const int p = g.pitch;
    const size_t pl = g.plane;
    const double gamma = P.gamma;

    // an earlier stage of this step met an invalid state: this one stores nothing (the flag is raised
    // by launches, read here once per workgroup: every thread takes the same way)
    if (KIND != RK_FIRST && t == 0) skip_s = *(volatile int *)flag & 1;

    // ---- phase 0: the stage state -> Q for the tile + 4-cell apron ----------------------------
    bool bad = false;
    {
        constexpr int NIT = (RQN + RNT - 1) / RNT;
        Cons Ul[NIT];
        size_t ks[NIT];
        bool act[NIT], interior[NIT];
#pragma unroll
        for (int n = 0; n < NIT; n++) {
            const int idx = t + n * RNT;
            act[n] = idx < RQN;
            const int ii = act[n] ? idx : t;       // idle lanes re-read their first cell
            const int r = ii / RQW, c = ii - r * RQW;
            int gi = i0 - 4 + r, gj = j0 - 4 + c;
            gi = (gi < g.qx) ? gi : g.qx - 1;   // ragged last tiles: clamp, unused
            gj = (gj < g.qy) ? gj : g.qy - 1;
            const unsigned sd = (gi < g.ilo ? 1u : 0u) | (gi > g.ihi ? 2u : 0u) | (gj < g.jlo ? 4u : 0u) |
                                (gj > g.jhi ? 8u : 0u);
            interior[n] = (sd == 0);
            if (KIND == RK_FIRST) {
                const size_t k = (size_t)gi * p + gj;
                ks[n] = k;
                Ul[n] = Cons{Uin[k], Uin[pl + k], Uin[2 * pl + k], Uin[3 * pl + k]};
            } else {
                // (the image of a ghost cell is an interior cell of y_0 and of every k_j: x rule, then
                // y rule, as fill_BC_all would have left the stage state's ghost cells)
                const int si = bc_src(P.mr, gi, g.ilo, g.ihi), sj = bc_src(P.mc, gj, g.jlo, g.jhi);
                const size_t k = (size_t)si * p + sj;
                ks[n] = k;
                Cons U{Uin[k], Uin[pl + k], Uin[2 * pl + k], Uin[3 * pl + k]};
                const double *K = P.rk_k + k;
#pragma unroll
                for (int jn = 0; jn < 3; jn++) {
                    if (jn < P.rk_n && P.rk_a[jn] != 0.0) {
                        const double w = dt * P.rk_a[jn];      // integration.py:116
                        const double *Kj = K + (size_t)(4 * jn) * pl;
                        U.d += w * Kj[0]; U.E += w * Kj[pl]; U.mx += w * Kj[2 * pl]; U.my += w * Kj[3 * pl];
                    }
                }
                U.d = odd_sides(P.odd & sd) ? -U.d : U.d;
                U.E = odd_sides((P.odd >> 4) & sd) ? -U.E : U.E;
                U.mx = odd_sides((P.odd >> 8) & sd) ? -U.mx : U.mx;
                U.my = odd_sides((P.odd >> 12) & sd) ? -U.my : U.my;
                Ul[n] = U;
            }
        }
#pragma unroll
        for (int n = 0; n < NIT; n++) {
            const int idx = t + n * RNT;
            const int r = idx / RQW, c = idx - r * RQW;
            Cons U = Ul[n];
            const bool dnan = nan_bits(U.d);      // np.maximum keeps a NaN: the floor must not launder it
            bool floored = false;
            if (interior[n]) {                    // clean_state
                const double dn = fmax(U.d, P.small_dens);
                floored = (dn != U.d);
                U.d = dn;
            }
            bool ok;
            const Prim q = cons_to_prim_nb(U, gamma, ok);
            if (act[n] && interior[n] && (!ok || dnan)) bad = true;
            // clean_state works in place -- in a cell that passes: a rejected cell stays as it was handed
            // over.  Only the tile that owns the cell stores; a neighbouring tile that reads the cell
            // meanwhile applies the floor itself (above): the same value either way.
            if (KIND == RK_FIRST && act[n] && floored && ok && !dnan && r >= 4 && r < 4 + RTI && c >= 4 &&
                c < 4 + RTJ)
                const_cast<double *>(Uin)[ks[n]] = U.d;
            if (act[n]) {
                Q[idx] = q.r; Q[RQN + idx] = q.u; Q[2 * RQN + idx] = q.v; Q[3 * RQN + idx] = q.p;
                if (r >= 3 && r < 3 + RBI && c >= 3 && c < 3 + RBJ) {
                    const int tt = (r - 3) * RBJ + (c - 3);
                    UC[tt] = U.E; UC[RNT + tt] = U.mx; UC[2 * RNT + tt] = U.my;
                }
            }
        }
    }
    if (bad) atomicOr(flag, 1);
    __syncthreads();
    const bool skip = (KIND != RK_FIRST) && skip_s != 0;

    // ---- phase 1: xi, limited slopes, face states of the thread's own cell (k_xi, k_rk_states) ----
    const int qc = (ti + 3) * RQW + (tj + 3);   // own cell in the Q tile
    Cons XM, YM;
    {
        const double *Qu = Q + RQN, *Qv = Q + 2 * RQN, *Qp = Q + 3 * RQN;
        double xi = 1.0;
        if (P.use_flattening) {
            // flatten_multid (reconstruction.py:167-183): own coefficient and the one of the UPWIND
            // neighbour (w.r.t. the pressure gradient) in each direction
            const int sx = (Qp[qc + RQW] - Qp[qc - RQW] > 0) ? -RQW : RQW;
            const int sy = (Qp[qc + 1] - Qp[qc - 1] > 0) ? -1 : 1;
            const int cx = qc + sx, cy = qc + sy;
            const double xix = flatten_1d(Qp[qc - 2 * RQW], Qp[qc - RQW], Qp[qc + RQW], Qp[qc + 2 * RQW],
                                          Qu[qc - RQW], Qu[qc + RQW], P.z0, P.z1, P.delta);
            const double px = flatten_1d(Qp[cx - 2 * RQW], Qp[cx - RQW], Qp[cx + RQW], Qp[cx + 2 * RQW],
                                         Qu[cx - RQW], Qu[cx + RQW], P.z0, P.z1, P.delta);
            const double xiy = flatten_1d(Qp[qc - 2], Qp[qc - 1], Qp[qc + 1], Qp[qc + 2], Qv[qc - 1],
                                          Qv[qc + 1], P.z0, P.z1, P.delta);
            const double py = flatten_1d(Qp[cy - 2], Qp[cy - 1], Qp[cy + 1], Qp[cy + 2], Qv[cy - 1],
                                         Qv[cy + 1], P.z0, P.z1, P.delta);
            xi = fmin(fmin(xix, px), fmin(xiy, py));
        }
        double q0[4], dqx[4], dqy[4];
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const double *a = Q + n * RQN;
            q0[n] = a[qc];
            dqx[n] = xi * limited_slope(a[qc - 2 * RQW], a[qc - RQW], a[qc], a[qc + RQW], a[qc + 2 * RQW],
                                        P.limiter);
            dqy[n] = xi * limited_slope(a[qc - 2], a[qc - 1], a[qc], a[qc + 1], a[qc + 2], P.limiter);
        }
        // fluxes.py:107-140: V_l[i+1] = q + ld/2 (the cell's upper face), V_r[i] = q - ld/2
        auto face = [&](const double *d, double sgn) {
            return prim_to_cons(Prim{q0[0] + sgn * 0.5 * d[0], q0[1] + sgn * 0.5 * d[1],
                                     q0[2] + sgn * 0.5 * d[2], q0[3] + sgn * 0.5 * d[3]}, gamma);
        };
        XM = face(dqx, -1.0);
        YM = face(dqy, -1.0);
        rkt_put(S, t, face(dqx, 1.0));
        rkt_put(SY, t, face(dqy, 1.0));
        D[t] = div_u_vertex(Qu[qc], Qu[qc - 1], Qu[qc - RQW], Qu[qc - RQW - 1], Qv[qc], Qv[qc - RQW],
                            Qv[qc - 1], Qv[qc - RQW - 1], P.dx, P.dy);
    }
    __syncthreads();

    // ---- phase 2: Riemann problems + artificial viscosity on the cell's lower faces (k_rk_flux) ----
    // (threads of the first row / column have no lower neighbour in the tile: their faces belong to
    // the neighbouring tile, what they compute here is never read)
    const Cons Uc{Q[qc], UC[t], UC[RNT + t], UC[2 * RNT + t]};
    Cons Fx, Fy;
    {
        const int tx = (ti >= 1) ? t - RBJ : t, ty = (tj >= 1) ? t - 1 : t;
        const double d00 = D[t];
        Fx = from_nf(riemann_face<SOLVER>(to_nf(rkt_get(S, tx), true), to_nf(XM, true), gamma, true,
                                          P.solid_xl && i == g.ilo), true);
        double avx = 0.0;
        if (i <= g.ihi || P.avx_hi) {
            const double d01 = D[(tj < RBJ - 1) ? t + 1 : t];
            avx = P.cvisc * fmax(-(0.5 * (d00 + d01)) * P.dx, 0.0);
        }
        rkt_avisc(Fx, avx, Cons{Q[(ti >= 1) ? qc - RQW : qc], UC[tx], UC[RNT + tx], UC[2 * RNT + tx]}, Uc);
        Fy = from_nf(riemann_face<SOLVER>(to_nf(rkt_get(SY, ty), false), to_nf(YM, false), gamma, false,
                                          P.solid_yl && j == g.jlo), false);
        double avy = 0.0;
        if (j <= g.jhi || P.avy_hi) {
            const double d10 = D[(ti < RBI - 1) ? t + RBJ : t];
            avy = P.cvisc * fmax(-(0.5 * (d00 + d10)) * P.dy, 0.0);
        }
        rkt_avisc(Fy, avy, Cons{Q[(tj >= 1) ? qc - 1 : qc], UC[ty], UC[RNT + ty], UC[2 * RNT + ty]}, Uc);
    }
    __syncthreads();        // every upper face state has been read: the fluxes take their place
    rkt_put(S, t, Fx);
    rkt_put(SY, t, Fy);
    __syncthreads();

    // ---- phase 3: k = (Fx[i] - Fx[i+1])/dx + (Fy[j] - Fy[j+1])/dy + S (k_rk_rhs) ----------------
    double cfl = INFINITY;
    if (ti >= 1 && ti <= RBI - 2 && tj >= 1 && tj <= RBJ - 2 && i <= g.ihi && j <= g.jhi && !skip) {
        const Cons Fxh = rkt_get(S, t + RBJ), Fyh = rkt_get(SY, t + 1);
        Cons kk;
        kk.d = rkt_div(Fx.d - Fxh.d, P.dx) + rkt_div(Fy.d - Fyh.d, P.dy);
        kk.E = rkt_div(Fx.E - Fxh.E, P.dx) + rkt_div(Fy.E - Fyh.E, P.dy);
        kk.mx = rkt_div(Fx.mx - Fxh.mx, P.dx) + rkt_div(Fy.mx - Fyh.mx, P.dy);
        kk.my = rkt_div(Fx.my - Fxh.my, P.dx) + rkt_div(Fy.my - Fyh.my, P.dy);
        // planes: density, energy, x-momentum, y-momentum; S = (0, ymom g, 0, rho g)
        // (no heating profile on this kernel: its term is rho * 0 * 0)
        kk.d = kk.d + 0.0;
        kk.E = kk.E + (Uc.my * P.grav + Uc.d * P.heat_rate * 0.0);
        kk.mx = kk.mx + 0.0;
        kk.my = kk.my + Uc.d * P.grav;
        const size_t k = (size_t)i * p + j;
        if (KIND != RK_LAST) {
            Kout[k] = kk.d; Kout[pl + k] = kk.E; Kout[2 * pl + k] = kk.mx; Kout[3 * pl + k] = kk.my;
        } else {
            // integration.py:120-129: y_0 += dt b_s k_s, s = 0 ... -- the earlier increments from
            // memory, the last one is kk; then the CFL quantity of compressible_rk/simulation.py:46-56
            Cons Y{Uin[k], Uin[pl + k], Uin[2 * pl + k], Uin[3 * pl + k]};
#pragma unroll
            for (int sg = 0; sg < 3; sg++) {
                if (sg < P.rk_nb - 1 && P.rk_b[sg] != 0.0) {
                    const double w = dt * P.rk_b[sg];
                    const double *Ks = P.rk_k + (size_t)(4 * sg) * pl + k;
                    Y.d += w * Ks[0]; Y.E += w * Ks[pl]; Y.mx += w * Ks[2 * pl]; Y.my += w * Ks[3 * pl];
                }
            }
            if (P.rk_b[P.rk_nb - 1] != 0.0) {
                const double w = dt * P.rk_b[P.rk_nb - 1];
                Y.d += w * kk.d; Y.E += w * kk.E; Y.mx += w * kk.mx; Y.my += w * kk.my;
            }
            double *O = P.rk_out + k;
            O[0] = Y.d; O[pl] = Y.E; O[2 * pl] = Y.mx; O[3 * pl] = Y.my;
#if PYRO_FAST
            double ax, ay;
            cfl_speeds(Y, gamma, ax, ay);
            cfl = pdiv(1.0, pdiv(ax, P.dx) + pdiv(ay, P.dy));
#else
            // k_rk_cfl
            const double u = Y.mx / Y.d, v = Y.my / Y.d;
            const double e = (Y.E - 0.5 * Y.d * (u * u + v * v)) / Y.d;
            const double pr = Y.d * e * (gamma - 1.0);
            const double cs = sqrt(gamma * pr / Y.d);
            cfl = 1.0 / ((fabs(u) + cs) / P.dx + (fabs(v) + cs) / P.dy);
#endif
        }
    }
    if (KIND == RK_LAST) {
        cfl = block_reduce_min(cfl);
        if (t == 0) partial[tile] = cfl;
    }
}

void rk_tile_geometry(int nx, int ny, int *tx, int *ty, int *ntiles)
{
    *tx = RTI;
    *ty = RTJ;
    *ntiles = ((nx + RTI - 1) / RTI) * ((ny + RTJ - 1) / RTJ);
}

// compressible_rk: the WHOLE Runge-Kutta step of compressible_rk/simulation.py:58-104 in nstages
// launches of the tile kernel above -- stage 0 on the filled state (density floor in place), every
// later stage with its start built at load and its ghost cells read through the boundary rules, the
// last one storing y_0 + dt sum_s b_s k_s into the second buffer (ghost frame carried over, buffers
// swapped) and leaving the CFL partials of the new state.  Signature and protocol of
// comp_rk_step_wave (comp_wave.hip).
// a: nstages x nstages, row-major (Butcher tableau, strictly lower triangular); b: nstages.
// S == nullptr: dt by value, flag and minimum read back (single step); S != nullptr: a step of a
// device-side run (pyrohip_comp_rk_evolve), dt from *S, *dmin_out = device address of the minimum.
int comp_rk_step_tile(pyrohip_state *s, const pyrohip_comp_params *p, pyrohip_state *kst, int nstages,
                      const double *a, const double *b, double dt, const StepScalars *S,
                      const double **dmin_out)
{
    pyrohip_ctx *c = s->ctx;
    const Geom &g = s->g;
    FP P;
    double *Uin, *Unew;
    PYRO_TRY(fused_prepare(s, p, dt, P, Uin, Unew, S == nullptr, true));
    int tx, ty;
    rk_tile_geometry(g.nx, g.ny, &tx, &ty, &P.ntiles);
    P.ntj = (g.ny + RTJ - 1) / RTJ;
    const int nt = P.ntiles;
    PYRO_TRY(c->reduce.ensure((nt + kMinStageBlocks + 2) * sizeof(double)));
    double *part = (double *)c->reduce.p;
    using KernelT = void (*)(const double *, double *, Geom, FP, int *, double *, const StepScalars *);
    static const KernelT kernels[3][3] = {
        {k_rk_tile<0, RK_FIRST>, k_rk_tile<0, RK_MIDDLE>, k_rk_tile<0, RK_LAST>},
        {k_rk_tile<1, RK_FIRST>, k_rk_tile<1, RK_MIDDLE>, k_rk_tile<1, RK_LAST>},
        {k_rk_tile<2, RK_FIRST>, k_rk_tile<2, RK_MIDDLE>, k_rk_tile<2, RK_LAST>}};
#ifndef PYRO_EMU
    static bool attr_set = false;
    if (!attr_set) {
        for (int sv = 0; sv < 3; sv++)
            for (int kd = 0; kd < 3; kd++)
                PYRO_CHECK_HIP(hipFuncSetAttribute((const void *)kernels[sv][kd],
                                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)RLDS_BYTES));
        attr_set = true;
    }
#endif
    const int solver = (p->riemann == 1 || p->riemann == 2) ? p->riemann : 0;
    const dim3 grid(nt), block(RBJ, RBI);
    // stage 0: the state itself, ghost cells filled in memory (they stay the state's "stale" ghost
    // cells after the step, like the reference's)
    // (a device-side run has filled the frames of both buffers with the launch of its dt policy:
    // evolve.hip: k_fill_frame2_policy)
    const bool prefilled = s->frame_prefilled;
    s->frame_prefilled = false;
    if (!prefilled) PYRO_TRY(pyrohip_fill_bc(s, -1));
    PYRO_LAUNCH(c, "k_rk_tile", kernels[solver][RK_FIRST], grid, block, RLDS_BYTES, (const double *)Uin, kst->d, g,
                P, s->d_flag, part, S);
    P.mr = bc_map(g.ilo, g.ihi, g.ng, s->bc[0], s->bc[1], true);
    P.mc = bc_map(g.jlo, g.jhi, g.ng, s->bc[2], s->bc[3], true);
    for (int n = 0; n < 4; n++)
        for (int sd = 0; sd < 4; sd++)
            if (s->bc[n * 4 + sd] == PYROHIP_BC_REFLECT_ODD) P.odd |= 1u << (4 * n + sd);
    P.rk_k = kst->d;
    for (int st = 1; st < nstages; st++) {
        P.rk_n = st;
        for (int j = 0; j < 3; j++) P.rk_a[j] = (j < st) ? a[st * nstages + j] : 0.0;
        P.rk_final = (st == nstages - 1) ? 1 : 0;
        P.rk_nb = nstages;
        for (int j = 0; j < 4; j++) P.rk_b[j] = (j < nstages) ? b[j] : 0.0;
        P.rk_out = Unew;
        PYRO_LAUNCH(c, "k_rk_tile", kernels[solver][P.rk_final ? RK_LAST : RK_MIDDLE], grid, block, RLDS_BYTES,
                    (const double *)Uin, kst->d + (size_t)(4 * st) * g.plane, g, P, s->d_flag, part, S);
    }
    PYRO_CHECK_HIP(hipGetLastError());
    if (!prefilled) state_copy_frame4(s);  // ghost frame of the state -> the new buffer
    s->cfl_is_global = false;
    if (S && nt <= 128 * kMinStageBlocks) {
        // device-side run: the next policy launch takes the minimum of the partials itself (fused_tail)
        s->pend_part = part;
        s->pend_n = nt;
        state_swap_alt(s);
        *dmin_out = part + nt + kMinStageBlocks;
        return 0;
    }
    const double *dmin = launch_min_reduce(c->stream, part, nt);
    if (S) { state_swap_alt(s); *dmin_out = dmin; return 0; }
    const int rc = fused_sync(s, dmin);   // flag + minimum read back; swap if the state was valid
    if (rc == 0) s->cfl_kind = 1;         // (the minimum is compressible_rk's CFL quantity)
    return rc;
}

}  // namespace PYRO_NS
}  // namespace pyro
