// burgers: the whole unsplit CTU step of (u, v) in ONE launch, and the stepping loop that runs it
// without a host round trip per step.
//
//   pyro/burgers/burgers_interface.py:4-312   edge states, transverse terms, riemann / upwind
//   pyro/burgers/simulation.py:37-117         method_compute_timestep, evolve
//
// k_bg_tile computes what the four staged launches of incompressible.hip (k_bg_hat, k_bg_trans,
// k_bg_mac, k_bg_update) compute, with the same per-cell functions (bg_states.h), operation by
// operation: compiled with -ffp-contract=off the new level is theirs bit for bit.  A workgroup
// owns a BG_TI x BG_TJ tile of the interior, j (contiguous) across the lanes:
//   1. u, v of the tile and an apron of 3 cells -> LDS (a cell's update reads the face's neighbour
//      cell, its transverse neighbours and their 5-point slopes: 3 cells in each direction, so the
//      outermost of the ng = 4 ghost cells is never read);
//   2. limited slopes and the eight hat states of every cell of the tile grown by one -> LDS;
//   3. the transverse terms of those cells (registers), then added to the hat states in place;
//   4. per interior cell the MAC velocities and fluxes of its four faces (each face is evaluated
//      by both its cells: a few selects, instead of four more LDS planes and a barrier) and the
//      update, written to the state's OTHER buffer;
//   5. the workgroup's CFL partial min(dx / max(max|u_new|, SMALL), dy / max(max|v_new|, SMALL)).
// LDS: 2 x 22 x 38 + 8 x 18 x 34 doubles = 52 544 B (+ 128 B of the block reduction): three
// workgroups per CU.  Nothing intermediate goes to memory.
// The workgroups behind the tiles carry the ghost frame over (the staged step updates in place:
// its ghost cells keep the boundary fill of the state before the step, which the tracers read).
#include "common.h"
#include "reduce.h"
#include "stencil.h"
#include "bg_states.h"

namespace pyro {

constexpr int BG_TI = 16, BG_TJ = 32, BG_H = 3, BG_THREADS = 256;
constexpr int BG_UH = BG_TI + 2 * BG_H, BG_UW = BG_TJ + 2 * BG_H;   // u, v with apron
constexpr int BG_BH = BG_TI + 2, BG_BW = BG_TJ + 2;                 // tile grown by one: the states
constexpr int BG_NB = BG_BH * BG_BW;
constexpr int BG_TPC = (BG_NB + BG_THREADS - 1) / BG_THREADS;       // cells of the grown tile per thread
constexpr double BG_SMALL = 1.e-12;                                 // simulation_null.py: self.SMALL
// planes of the states in LDS (the order of incompressible.hip's work planes)
enum { H_UXL, H_UXR, H_UYL, H_UYR, H_VXL, H_VXR, H_VYL, H_VYR };

struct BGT {
    double dx, dy, dtdx, dtdy;
    int gx, gy;          // tiles across (columns) / down (rows)
    int ntile_blocks;    // workgroups of the tiles (xcd_grid_1d); the frame pieces follow
    int copy_frame;      // carry the ghost frame over to the new buffer
};

// the ghost cells of piece b (frame_pieces, common.h) of two planes, copied
__device__ __forceinline__ void bg_copy_frame_piece(const double *__restrict__ uin, const double *__restrict__ vin,
                                                    double *__restrict__ uout, double *__restrict__ vout,
                                                    const Geom &g, int b, int t)
{
    const int ng = g.ng, ncolb = (g.qy + 255) / 256, nrowb = 2 * ng * ncolb;
    int i, j;
    if (b < nrowb) {
        const int gr = b / ncolb;
        i = gr < ng ? gr : g.ihi + 1 + (gr - ng);
        j = (b % ncolb) * 256 + t;
        if (j >= g.qy) return;
    } else {
        const int rpb = 256 / (2 * ng);
        if (t >= rpb * 2 * ng) return;
        i = g.ilo + (b - nrowb) * rpb + t / (2 * ng);
        if (i > g.ihi) return;
        const int gc = t % (2 * ng);
        j = gc < ng ? gc : g.jhi + 1 + (gc - ng);
    }
    const size_t k = (size_t)i * g.pitch + j;
    uout[k] = uin[k];
    vout[k] = vin[k];
}

// S (device-side stepping, pyrohip_bg_evolve): this step's dt / dx, dt / dy from the step scalars
// the policy kernel left; nothing is stored when the step does not run.  part: one CFL partial per tile
template <int LIM>
__global__ __launch_bounds__(BG_THREADS) void k_bg_tile(const double *__restrict__ uin,
                                                        const double *__restrict__ vin,
                                                        double *__restrict__ uout, double *__restrict__ vout,
                                                        Geom g, BGT P, const StepScalars *__restrict__ S,
                                                        double *__restrict__ part)
{
    __shared__ double U[BG_UH * BG_UW], V[BG_UH * BG_UW];
    __shared__ double H[8][BG_NB];
    double dtdx = P.dtdx, dtdy = P.dtdy;
    if (S != nullptr) {
        if (!S->active) return;
        dtdx = S->dtdx; dtdy = S->dtdy;
    }
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= P.ntile_blocks) {
        if (P.copy_frame) bg_copy_frame_piece(uin, vin, uout, vout, g, (int)blockIdx.x - P.ntile_blocks, tid);
        return;
    }
    int bx, by;
    if (!xcd_block_2d(P.gx, P.gy, bx, by)) return;
    const int I0 = g.ilo + by * BG_TI, J0 = g.jlo + bx * BG_TJ;     // first cell of the tile

    // ---- 1. u, v with the apron (ghost cells as filled; a ragged tile's cells beyond the array
    // feed discarded cells only: any address inside)
    for (int n = tid; n < BG_UH * BG_UW; n += BG_THREADS) {
        const int r = n / BG_UW, c = n - r * BG_UW;
        int i = I0 - BG_H + r, j = J0 - BG_H + c;
        i = i > g.qx - 1 ? g.qx - 1 : i;
        j = j > g.qy - 1 ? g.qy - 1 : j;
        const size_t k = (size_t)i * g.pitch + j;
        U[n] = uin[k];
        V[n] = vin[k];
    }
    __syncthreads();

    // ---- 2. hat states of the tile grown by one (get_interface_states)
    for (int n = tid; n < BG_NB; n += BG_THREADS) {
        const int r = n / BG_BW, c = n - r * BG_BW;
        const int k = (r + BG_H - 1) * BG_UW + c + BG_H - 1;
        const double uc = U[k], vc = V[k];
        const double ldux = limited_slope(U[k - 2 * BG_UW], U[k - BG_UW], uc, U[k + BG_UW], U[k + 2 * BG_UW], LIM);
        const double ldvx = limited_slope(V[k - 2 * BG_UW], V[k - BG_UW], vc, V[k + BG_UW], V[k + 2 * BG_UW], LIM);
        const double lduy = limited_slope(U[k - 2], U[k - 1], uc, U[k + 1], U[k + 2], LIM);
        const double ldvy = limited_slope(V[k - 2], V[k - 1], vc, V[k + 1], V[k + 2], LIM);
        const BgHat hu = bg_hat(uc, ldux, lduy, uc, vc, dtdx, dtdy);
        const BgHat hv = bg_hat(vc, ldvx, ldvy, uc, vc, dtdx, dtdy);
        H[H_UXL][n] = hu.xl; H[H_UXR][n] = hu.xr; H[H_UYL][n] = hu.yl; H[H_UYR][n] = hu.yr;
        H[H_VXL][n] = hv.xl; H[H_VXR][n] = hv.xr; H[H_VYL][n] = hv.yl; H[H_VYR][n] = hv.yr;
    }
    __syncthreads();

    // ---- 3. transverse terms (apply_transverse_corrections): x states of the cells in the tile's
    // columns, y states of those in its rows (the others would need hat states beyond the grown
    // tile and reach no face of the tile)
    double tu[BG_TPC], tv[BG_TPC], su[BG_TPC], sv[BG_TPC];
#pragma unroll
    for (int q = 0; q < BG_TPC; q++) {
        const int n = tid + q * BG_THREADS;
        tu[q] = tv[q] = su[q] = sv[q] = 0.0;
        if (n >= BG_NB) continue;
        const int r = n / BG_BW, c = n - r * BG_BW;
        if (c >= 1 && c <= BG_TJ)
            bg_transverse(dtdy, H[H_VYL][n - 1], H[H_VYR][n], H[H_VYL][n], H[H_VYR][n + 1],
                          H[H_UYL][n - 1], H[H_UYR][n], H[H_UYL][n], H[H_UYR][n + 1],
                          H[H_VYL][n - 1], H[H_VYR][n], H[H_VYL][n], H[H_VYR][n + 1], tu[q], tv[q]);
        if (r >= 1 && r <= BG_TI)
            bg_transverse(dtdx, H[H_UXL][n - BG_BW], H[H_UXR][n], H[H_UXL][n], H[H_UXR][n + BG_BW],
                          H[H_VXL][n - BG_BW], H[H_VXR][n], H[H_VXL][n], H[H_VXR][n + BG_BW],
                          H[H_UXL][n - BG_BW], H[H_UXR][n], H[H_UXL][n], H[H_UXR][n + BG_BW], sv[q], su[q]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < BG_TPC; q++) {
        const int n = tid + q * BG_THREADS;
        if (n >= BG_NB) continue;
        const int r = n / BG_BW, c = n - r * BG_BW;
        if (c >= 1 && c <= BG_TJ) {
            H[H_UXL][n] = H[H_UXL][n] + tu[q]; H[H_UXR][n] = H[H_UXR][n] + tu[q];
            H[H_VXL][n] = H[H_VXL][n] + tv[q]; H[H_VXR][n] = H[H_VXR][n] + tv[q];
        }
        if (r >= 1 && r <= BG_TI) {
            H[H_VYL][n] = H[H_VYL][n] + sv[q]; H[H_VYR][n] = H[H_VYR][n] + sv[q];
            H[H_UYL][n] = H[H_UYL][n] + su[q]; H[H_UYR][n] = H[H_UYR][n] + su[q];
        }
    }
    __syncthreads();

    // ---- 4. MAC velocities, fluxes and the update (riemann_and_upwind, construct_unsplit_fluxes,
    // simulation.py:96-101) of the tile's cells that lie in the interior
    double mu = 0.0, mv = 0.0;
    for (int n = tid; n < BG_TI * BG_TJ; n += BG_THREADS) {
        const int r = n / BG_TJ, c = n - r * BG_TJ;
        const int i = I0 + r, j = J0 + c;
        if (i > g.ihi || j > g.jhi) continue;
        const int m = (r + 1) * BG_BW + c + 1;
        const int k = (r + BG_H) * BG_UW + c + BG_H;
        // x faces: the cell's low one (left state from the cell below) and its high one
        const double um0 = bg_mac(H[H_UXL][m - BG_BW], H[H_UXR][m]);
        const double um1 = bg_mac(H[H_UXL][m], H[H_UXR][m + BG_BW]);
        const double fxu0 = bg_flux(H[H_UXL][m - BG_BW], H[H_UXR][m], um0);
        const double fxu1 = bg_flux(H[H_UXL][m], H[H_UXR][m + BG_BW], um1);
        const double fxv0 = bg_flux(H[H_VXL][m - BG_BW], H[H_VXR][m], um0);
        const double fxv1 = bg_flux(H[H_VXL][m], H[H_VXR][m + BG_BW], um1);
        // y faces
        const double vm0 = bg_mac(H[H_VYL][m - 1], H[H_VYR][m]);
        const double vm1 = bg_mac(H[H_VYL][m], H[H_VYR][m + 1]);
        const double fyu0 = bg_flux(H[H_UYL][m - 1], H[H_UYR][m], vm0);
        const double fyu1 = bg_flux(H[H_UYL][m], H[H_UYR][m + 1], vm1);
        const double fyv0 = bg_flux(H[H_VYL][m - 1], H[H_VYR][m], vm0);
        const double fyv1 = bg_flux(H[H_VYL][m], H[H_VYR][m + 1], vm1);
        const double un = U[k] + dtdx * (fxu0 - fxu1) + dtdy * (fyu0 - fyu1);
        const double vn = V[k] + dtdx * (fxv0 - fxv1) + dtdy * (fyv0 - fyv1);
        const size_t ko = (size_t)i * g.pitch + j;
        uout[ko] = un;
        vout[ko] = vn;
        mu = fmax(mu, fabs(un));
        mv = fmax(mv, fabs(vn));
    }

    // ---- 5. the CFL partial of the tile (simulation.py:37-51 on the new level's interior)
    if (part != nullptr) {
        mu = block_reduce_max(mu);
        mv = block_reduce_max(mv);
        if (tid == 0) part[by * P.gx + bx] = fmin(P.dx / fmax(mu, BG_SMALL), P.dy / fmax(mv, BG_SMALL));
    }
}

// the same partials over the interior of the state as handed over (first step of a call): for the
// four index-map boundary kinds every ghost cell is +- an interior cell, so the interior maxima are
// the whole-array maxima method_compute_timestep takes after the fill
__global__ __launch_bounds__(BG_THREADS) void k_bg_cfl(const double *__restrict__ u, const double *__restrict__ v,
                                                       Geom g, BGT P, double *__restrict__ part)
{
    const int bx = (int)blockIdx.x % P.gx, by = (int)blockIdx.x / P.gx;
    const int I0 = g.ilo + by * BG_TI, J0 = g.jlo + bx * BG_TJ;
    double mu = 0.0, mv = 0.0;
    for (int n = threadIdx.x; n < BG_TI * BG_TJ; n += BG_THREADS) {
        const int r = n / BG_TJ, c = n - r * BG_TJ;
        const int i = I0 + r, j = J0 + c;
        if (i > g.ihi || j > g.jhi) continue;
        const size_t k = (size_t)i * g.pitch + j;
        mu = fmax(mu, fabs(u[k]));
        mv = fmax(mv, fabs(v[k]));
    }
    mu = block_reduce_max(mu);
    mv = block_reduce_max(mv);
    if (threadIdx.x == 0) part[blockIdx.x] = fmin(P.dx / fmax(mu, BG_SMALL), P.dy / fmax(mv, BG_SMALL));
}

static BGT bg_tiles(const Geom &g, double dx, double dy, double dt)
{
    BGT P;
    P.dx = dx; P.dy = dy; P.dtdx = dt / dx; P.dtdy = dt / dy;
    P.gx = (g.ny + BG_TJ - 1) / BG_TJ;
    P.gy = (g.nx + BG_TI - 1) / BG_TI;
    P.ntile_blocks = xcd_grid_1d(P.gx, P.gy);
    P.copy_frame = 0;
    return P;
}

static int bg_check(pyrohip_state *s, int iu, int iv, double dx, double dy, int limiter)
{
    PYRO_REQUIRE(s, "NULL state");
    PYRO_REQUIRE(s->nvar == 2 && ((iu == 0 && iv == 1) || (iu == 1 && iv == 0)),
                 "the one-launch burgers step exchanges the state's two buffers: a state of exactly the two "
                 "velocity components");
    PYRO_REQUIRE(s->g.ng >= 4, "the CTU predictor needs ng >= 4");
    PYRO_REQUIRE(dx > 0 && dy > 0, "bad dx / dy");
    PYRO_REQUIRE(limiter >= 0 && limiter <= 2, "limiter must be 0, 1 or 2");
    return 0;
}

// one step by the one-launch kernel: new level into the second buffer, ghost frame carried over
// (unless the caller has filled both frames: frame_done), buffers exchanged
static int bg_step_tile(pyrohip_state *s, int iu, int iv, double dx, double dy, double dt, int limiter,
                        const StepScalars *S, double *part, bool frame_done)
{
    pyrohip_ctx *c = s->ctx;
    const Geom &g = s->g;
    PYRO_TRY(state_alt(s));
    BGT P = bg_tiles(g, dx, dy, dt);
    P.copy_frame = frame_done ? 0 : 1;
    const double *in = s->d;
    double *out = s->alt_base + geom_lead(g);
    const dim3 grid(P.ntile_blocks + (P.copy_frame ? frame_pieces(g) : 0)), block(BG_THREADS);
    using KernelT = void (*)(const double *, const double *, double *, double *, Geom, BGT, const StepScalars *,
                             double *);
    static const KernelT kernels[3] = {k_bg_tile<0>, k_bg_tile<1>, k_bg_tile<2>};
    PYRO_LAUNCH(c, "k_bg_tile", kernels[limiter], grid, block, 0, in + (size_t)iu * g.plane,
                in + (size_t)iv * g.plane, out + (size_t)iu * g.plane, out + (size_t)iv * g.plane, g, P, S, part);
    PYRO_CHECK_HIP(hipGetLastError());
    state_swap_alt(s);
    s->next_cfl_min = -1.0;
    s->ghost_by_rules = false;
    return 0;
}

}  // namespace pyro

using namespace pyro;

extern "C" {

int pyrohip_bg_step1(pyrohip_state *s, int iu, int iv, double dx, double dy, double dt, int limiter)
{
    PYRO_TRY(bg_check(s, iu, iv, dx, dy, limiter));
    PYRO_TRY(comm_wait_halo(s));
    return bg_step_tile(s, iu, iv, dx, dy, dt, limiter, nullptr, nullptr, false);
}

// Up to max_steps iterations of the burgers driver loop (pyro_sim.py:241-281 with burgers/
// simulation.py:37-117: ghost fill, CFL time step, evolve) without a host round trip per step: the
// run protocol of DESIGN.md 3.6.1 (evolve.hip) around k_bg_tile, whose workgroups leave the CFL
// partials the next policy call reduces.  Two launches per step (frames of both buffers + policy,
// the step) and the tracers' three.
int pyrohip_bg_evolve_p(pyrohip_state *s, int iu, int iv, double dx, double dy, int limiter, double cfl,
                        pyrohip_dt_policy *pol, int max_steps, int *steps_done, double *dts_out,
                        pyrohip_particles *particles, const pyrohip_particle_params *pparams)
{
    PYRO_TRY(bg_check(s, iu, iv, dx, dy, limiter));
    PYRO_REQUIRE(pol && steps_done && max_steps >= 1, "NULL argument / max_steps must be positive");
    PYRO_REQUIRE(!s->nb_set && !s->user_bc && !s->ramp_bc && !s->sph,
                 "device-side stepping: burgers runs on a single Cartesian domain with the standard boundary types");
    // from the second step on the CFL minimum is the step kernel's (interior of the new state):
    // equal to the reference's whole-array maxima only where every ghost cell is +- an interior cell
    for (int k = 0; k < 4 * s->nvar; k++)
        PYRO_REQUIRE(bc_is_index_map(s->bc[k], true),
                     "device-side stepping: outflow / reflect / periodic boundaries only");
    pyrohip_ctx *c = s->ctx;
    const Geom &g = s->g;
    PYRO_TRY(state_alt(s));     // (k_fill_frame2 writes the second buffer's frame)
    EvolveRun r;
    PYRO_TRY(evolve_bind_particles(r, s, particles, pparams, __func__));
    PYRO_TRY(evolve_open(r, s, pol, cfl, 3, 0.0, dx, dy, max_steps, false));
    // one partial per tile, sized BEFORE the first launch
    const BGT P = bg_tiles(g, dx, dy, 0.0);
    const int ntiles = P.gx * P.gy;
    PYRO_TRY(c->reduce.ensure((size_t)ntiles * sizeof(double)));
    double *part = (double *)c->reduce.p;
    r.dmin = &s->d_scal->min0;      // the cached minimum; every later policy call leaves its own there
    int rc = 0;
    for (int m = 0; m < max_steps && rc == 0; m++) {
        bool frame_done = false;
        if (m == 0) {      // the CFL minimum of the state as handed over
            rc = evolve_fill(r, true, &frame_done);          // pyro_sim.py:250: fill_BC_all
            if (rc) break;
            r.pend = nullptr;
            if (!r.min_cached) {
                PYRO_LAUNCH(c, "k_bg_cfl", k_bg_cfl, dim3(ntiles), dim3(BG_THREADS), 0,
                            (const double *)s->d + (size_t)iu * g.plane,
                            (const double *)s->d + (size_t)iv * g.plane, g, P, part);
                PYRO_CHECK_HIP(hipGetLastError());
                r.pend = part; r.npend = ntiles;
            }
            rc = evolve_policy(r, m);
        } else
            rc = evolve_between(r, m, true, true, &frame_done);
        if (rc) break;
        rc = bg_step_tile(s, iu, iv, dx, dy, 0.0, limiter, s->d_scal, part, frame_done);
        r.pend = part; r.npend = ntiles;
        if (rc == 0) rc = evolve_particles(r);
    }
    PYRO_TRY(rc);
    // (no burgers kernel raises the flag: only a bound particle set can end the run)
    return evolve_close(r, pol, steps_done, dts_out, true, false);
}

int pyrohip_bg_evolve(pyrohip_state *s, int iu, int iv, double dx, double dy, int limiter, double cfl,
                      pyrohip_dt_policy *pol, int max_steps, int *steps_done, double *dts_out)
{
    return pyrohip_bg_evolve_p(s, iu, iv, dx, dy, limiter, cfl, pol, max_steps, steps_done, dts_out, nullptr,
                               nullptr);
}

}  // extern "C"
