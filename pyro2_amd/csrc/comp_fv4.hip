// Fourth-order compressible hydro (McCorquodale & Colella 2011), the method-of-lines right-hand
// side of compressible_fv4 / compressible_sdc.
//
// Replaces (reference file:line)
//   pyro/compressible_fv4/simulation.py:21-66   Simulation.substep
//   pyro/compressible_fv4/fluxes.py:46-223      flux_cons, fluxes
//   pyro/mesh/fourth_order.py:8-235             states (limited 4th-order face states)
//   pyro/compressible/riemann.py:314-574        riemann_prim (CGF on primitive states)
//   pyro/mesh/fv.py:18-39                       to_centers / from_centers
//   pyro/compressible_sdc/simulation.py:48-127  the node update of the SDC sweep
//
// k_fv4_rhs: one workgroup per tile of TI x TJ cells, every intermediate in LDS.  The stencil
// radius of the scheme is 5 cells (face states read q_avg at -4 .. +3, q_avg reads the
// averages at +-1), so a tile loads the state on a (TI + 10) x (TJ + 10) window and works
// inward:
//   load (U, interior density floored; q_bar)  ->  U_cc, q_cc, q_avg; S at centres; xi_x, xi_y
//   ->  xi
//   ->  x faces: limited states, flattening, CGF  ->  F_x (face-centred + transverse
//       Laplacian + artificial viscosity)  ->  the same for y  ->  k = -div F + <S> - sponge
// The state is read once (plus the halo) and k written once.  k_fv4_prep runs in front of
// it: the density floor of the interior (written back, like clean_state) and the two
// cons_to_prim asserts, so that an invalid state leaves k untouched.
//
// Batches of steps on the device (pyrohip_comp_fv4_evolve / pyrohip_comp_sdc_evolve):
// comp_fv4_rhs_run is the two launches without the host side of the flag; k_fv4_stage_start,
// k_fv4_sdc_node and k_fv4_final form a stage / node / new state AND its ghost cells in one launch,
// with dt from the run's step scalars (the bit-faithful part at the end of the file: one instance
// serves both builds).
//
// This file is compiled twice (builds.h): PYRO_FAST=0 (-ffp-contract=off, the bit-faithful build) and
// PYRO_FAST=1 (-ffp-contract=fast); the entry points (comp_api.hip) dispatch on fast_math.  Exports:
// comp_units.h.
#include "builds.h"
#include "common.h"
#include "hydro.h"
#include "fv4_limit.h"
#include "reduce.h"

namespace pyro {
namespace PYRO_NS {
#include "comp_units.h"

namespace {

constexpr int TI = 8;            // tile rows (x, the slow index)
constexpr int TJ = 32;           // tile columns (y, contiguous in memory)
constexpr int NT = 512;          // threads per workgroup

// a tile-local cell box with an apron of H cells: a in [-H, TI + H), b in [-H, TJ + H)
template <int H>
struct Box {
    static constexpr int NI = TI + 2 * H, NJ = TJ + 2 * H, N = NI * NJ;
    static __device__ __forceinline__ int at(int a, int b) { return (a + H) * NJ + (b + H); }
};
using B5 = Box<5>;
using B4 = Box<4>;
using B2 = Box<2>;
using B1 = Box<1>;
// x faces f in [0, TI] on rows b in [-1, TJ]; y faces g in [0, TJ] on columns a in [-1, TI]
__device__ __forceinline__ int xf(int f, int b) { return f * (TJ + 2) + (b + 1); }
__device__ __forceinline__ int yf(int a, int g) { return (a + 1) * (TJ + 1) + g; }
constexpr int NQI = (TI + 1) * (TJ + 2) > (TI + 2) * (TJ + 1) ? (TI + 1) * (TJ + 2) : (TI + 2) * (TJ + 1);
constexpr int NFX = (TI + 1) * TJ, NFY = TI * (TJ + 1);

struct FP {   // kernel-side parameters
    double gamma, dx, dy, z0, z1, delta, small_dens, grav, heat_rate;
    const double *heat;
    int use_flattening;
    int sponge;
    double rho_begin, rho_full, tau;
};

__device__ __forceinline__ double floor_dens(double d, double small)
{
    return (d < small) ? small : d;     // np.maximum(d, small_dens); a NaN stays a NaN
}

// fluxes.py:12-38 in the face's (normal, transverse) frame; returns (d, E, mn, mt)
__device__ __forceinline__ void flux_cons_n(const PrimN &q, double gamma, double *F)
{
    F[0] = q.r * q.un;
    F[2] = q.r * (q.un * q.un) + q.p;
    F[3] = q.r * q.ut * q.un;
    F[1] = (q.p / (gamma - 1.0) + 0.5 * q.r * (q.un * q.un + q.ut * q.ut) + q.p) * q.un;
}

// (rho, u, v, p) plane order of the LDS primitive arrays; conserved planes: d, E, mx, my
enum { QR = 0, QU = 1, QV = 2, QP = 3 };

struct Lds {
    double U[4][B5::N];      // averages, the interior density floored
    double Qb[4][B5::N];     // q_bar
    double Qa[4][B4::N];     // q_avg (0 in the outermost ghost ring, as the reference's buf = 3)
    double S[2][B1::N];      // S[E], S[ymom] at cell centres
    double Xi[B1::N];        // flattening coefficient
    union {
        double Xd[2][B2::N];   // xi_x, xi_y
        double Qi[4][NQI];     // face-average primitive state (rho, u, v, p) of one sweep
    };
    double Fx[4][NFX];
    double Fy[4][NFY];
};

}  // namespace

// density floor of the interior (written back: clean_state modifies the stage state,
// fv4/simulation.py:24, through U.v() -- compressible/simulation.py:452-456 -- so the ghost cells
// keep their density) and the two cons_to_prim asserts of fluxes.py:80-81 (U_avg and the masked
// U_cc, interior only).
// flag |= 1 on an invalid state.
// S: the step scalars of a device-side run (nullptr: a single right-hand side) -- an iteration that
// does not advance (past tmax, after an invalid state) neither floors nor judges what it is given.
__global__ __launch_bounds__(256) void k_fv4_prep(double *__restrict__ U, Geom g, FP P,
                                                  int *__restrict__ flag, const StepScalars *__restrict__ S)
{
    if (S != nullptr && S->active == 0) return;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= g.qy) return;
    if (i < g.ilo || i > g.ihi || j < g.jlo || j > g.jhi) return;   // ghosts keep their density
    const size_t pl = g.plane;
    const size_t k = (size_t)i * g.pitch + j;
    const double d0 = U[k];
    const double d = floor_dens(d0, P.small_dens);
    if (d != d0) U[k] = d;
    bool ok_avg, ok_cc;
    const Cons Ua{d, U[pl + k], U[2 * pl + k], U[3 * pl + k]};
    (void)cons_to_prim(Ua, P.gamma, &ok_avg);
    // to_centers (fv.py:18-29) of the four variables, then the mask of fluxes.py:55-66
    const double dx2 = P.dx * P.dx, dy2 = P.dy * P.dy;
    double c[4];
#pragma unroll
    for (int n = 0; n < 4; n++) {
        const double *a = U + n * pl;
        double v = a[k], im = a[k - g.pitch], ip = a[k + g.pitch], jm = a[k - 1], jp = a[k + 1];
        if (n == 0) {   // the floored density of the interior neighbours (written by their threads)
            v = d;
            if (i > g.ilo) im = floor_dens(im, P.small_dens);
            if (i < g.ihi) ip = floor_dens(ip, P.small_dens);
            if (j > g.jlo) jm = floor_dens(jm, P.small_dens);
            if (j < g.jhi) jp = floor_dens(jp, P.small_dens);
        }
        const double lap = (im - 2 * v + ip) / dx2 + (jm - 2 * v + jp) / dy2;
        c[n] = v - dx2 * lap / 24.0;
    }
    const double rhoe = c[1] - 0.5 * (c[2] * c[2] + c[3] * c[3]) / c[0];
    const Cons Uc = (c[0] < 0 || rhoe < 0) ? Ua : Cons{c[0], c[1], c[2], c[3]};
    (void)cons_to_prim(Uc, P.gamma, &ok_cc);
    if (!(ok_avg && ok_cc)) atomicOr(flag, 1);
}

__global__ __launch_bounds__(NT) void k_fv4_rhs(const double *__restrict__ Ug, double *__restrict__ K,
                                                Geom g, FP P, const int *__restrict__ flag)
{
    if (*flag) return;     // invalid state: k stays as it was
    __shared__ Lds L;
    const int i0 = g.ilo + blockIdx.x * TI, j0 = g.jlo + blockIdx.y * TJ;
    const int t = threadIdx.x;
    const size_t pl = g.plane;
    const double dx2 = P.dx * P.dx, dy2 = P.dy * P.dy;

    // ---- 1. averages (density floored on the interior) and q_bar on the 5-cell apron (zero
    //         beyond the array) -----------------------------------------------------------------
    for (int e = t; e < B5::N; e += NT) {
        const int a = e / B5::NJ - 5, b = e % B5::NJ - 5;
        const int i = i0 + a, j = j0 + b;
        Cons u{0.0, 0.0, 0.0, 0.0};
        if (i >= 0 && i < g.qx && j >= 0 && j < g.qy) {
            const size_t k = (size_t)i * g.pitch + j;
            const bool inner = i >= g.ilo && i <= g.ihi && j >= g.jlo && j <= g.jhi;
            u = Cons{inner ? floor_dens(Ug[k], P.small_dens) : Ug[k], Ug[pl + k], Ug[2 * pl + k],
                     Ug[3 * pl + k]};
        }
        L.U[0][e] = u.d; L.U[1][e] = u.E; L.U[2][e] = u.mx; L.U[3][e] = u.my;
        const Prim q = cons_to_prim(u, P.gamma);
        L.Qb[QR][e] = q.r; L.Qb[QU][e] = q.u; L.Qb[QV][e] = q.v; L.Qb[QP][e] = q.p;
    }
    __syncthreads();

    // ---- 2. U_cc, q_cc, q_avg on the 4-cell apron; S at centres (1-cell apron); xi_x, xi_y ----
    for (int e = t; e < B4::N; e += NT) {
        const int a = e / B4::NJ - 4, b = e % B4::NJ - 4;
        const int i = i0 + a, j = j0 + b;
        const int c5 = B5::at(a, b);
        if (i < 1 || i > g.qx - 2 || j < 1 || j > g.qy - 2) {
#pragma unroll
            for (int n = 0; n < 4; n++) L.Qa[n][e] = 0.0;
            continue;
        }
        const int im = B5::at(a - 1, b), ip = B5::at(a + 1, b), jm = B5::at(a, b - 1), jp = B5::at(a, b + 1);
        double c[4];
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const double *A = L.U[n];
            const double lap = (A[im] - 2 * A[c5] + A[ip]) / dx2 + (A[jm] - 2 * A[c5] + A[jp]) / dy2;
            c[n] = A[c5] - dx2 * lap / 24.0;
        }
        if (a >= -1 && a <= TI && b >= -1 && b <= TJ) {
            // get_external_sources (compressible/simulation.py:127-128) + the heating profile,
            // on the unmasked centres
            const int c1 = B1::at(a, b);
            const double hp = P.heat ? P.heat[(size_t)i * g.pitch + j] : 0.0;
            L.S[0][c1] = c[3] * P.grav + c[0] * P.heat_rate * hp;
            L.S[1][c1] = c[0] * P.grav;
        }
        const double rhoe = c[1] - 0.5 * (c[2] * c[2] + c[3] * c[3]) / c[0];
        Cons uc{c[0], c[1], c[2], c[3]};
        if (c[0] < 0 || rhoe < 0) uc = Cons{L.U[0][c5], L.U[1][c5], L.U[2][c5], L.U[3][c5]};
        const Prim qc = cons_to_prim(uc, P.gamma);
        const double qcv[4] = {qc.r, qc.u, qc.v, qc.p};
        const double f = dx2 / 24.0;
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const double *Q = L.Qb[n];
            const double lap = (Q[im] - 2 * Q[c5] + Q[ip]) / dx2 + (Q[jm] - 2 * Q[c5] + Q[jp]) / dy2;
            double v = qcv[n] + f * lap;
            if ((n == QR || n == QP) && !(v > 0)) v = qcv[n];
            L.Qa[n][e] = v;
        }
    }
    for (int e = t; e < B2::N; e += NT) {
        const int a = e / B2::NJ - 2, b = e % B2::NJ - 2;
        const int i = i0 + a, j = j0 + b;
        double xx = 1.0, xy = 1.0;
        // reconstruction.flatten: evaluated on buf = 2, 1 elsewhere
        if (P.use_flattening && i >= g.ilo - 2 && i <= g.ihi + 2 && j >= g.jlo - 2 && j <= g.jhi + 2) {
            const double *p = L.Qb[QP];
            xx = flatten_1d(p[B5::at(a - 2, b)], p[B5::at(a - 1, b)], p[B5::at(a + 1, b)],
                            p[B5::at(a + 2, b)], L.Qb[QU][B5::at(a - 1, b)], L.Qb[QU][B5::at(a + 1, b)],
                            P.z0, P.z1, P.delta);
            xy = flatten_1d(p[B5::at(a, b - 2)], p[B5::at(a, b - 1)], p[B5::at(a, b + 1)],
                            p[B5::at(a, b + 2)], L.Qb[QV][B5::at(a, b - 1)], L.Qb[QV][B5::at(a, b + 1)],
                            P.z0, P.z1, P.delta);
        }
        L.Xd[0][e] = xx;
        L.Xd[1][e] = xy;
    }
    __syncthreads();

    // ---- 3. flatten_multid (reconstruction.py:167-183) on the 1-cell apron -------------------
    for (int e = t; e < B1::N; e += NT) {
        const int a = e / B1::NJ - 1, b = e % B1::NJ - 1;
        double xi = 1.0;
        if (P.use_flattening) {
            const double *p = L.Qb[QP];
            const double *X = L.Xd[0], *Y = L.Xd[1];
            const double px = (p[B5::at(a + 1, b)] - p[B5::at(a - 1, b)] > 0) ? X[B2::at(a - 1, b)]
                                                                                : X[B2::at(a + 1, b)];
            const double py = (p[B5::at(a, b + 1)] - p[B5::at(a, b - 1)] > 0) ? Y[B2::at(a, b - 1)]
                                                                                : Y[B2::at(a, b + 1)];
            xi = fmin(fmin(X[B2::at(a, b)], px), fmin(Y[B2::at(a, b)], py));
        }
        L.Xi[e] = xi;
    }
    __syncthreads();

    // ---- 4. x faces: states, flattening, riemann_prim ----------------------------------------
    for (int e = t; e < (TI + 1) * (TJ + 2); e += NT) {
        const int f = e / (TJ + 2), b = e % (TJ + 2) - 1;
        const double xl = L.Xi[B1::at(f - 1, b)], xr = L.Xi[B1::at(f, b)];
        double ql[4], qr[4];
#pragma unroll
        for (int n = 0; n < 4; n++) {
            double w[8];
#pragma unroll
            for (int m = 0; m < 8; m++) w[m] = L.Qa[n][B4::at(f - 4 + m, b)];
            double ar_l, al_f, ar_f, al_r;
            mc_limit(w, false, ar_l, al_f);          // cell f-1: al on face f
            mc_limit(w + 1, false, ar_f, al_r);      // cell f: ar on face f
            ql[n] = xl * al_f + (1.0 - xl) * w[3];
            qr[n] = xr * ar_f + (1.0 - xr) * w[4];
        }
        const PrimN s = cgf_prim(PrimN{ql[QR], ql[QU], ql[QV], ql[QP]}, PrimN{qr[QR], qr[QU], qr[QV], qr[QP]},
                                 P.gamma);
        L.Qi[QR][e] = s.r; L.Qi[QU][e] = s.un; L.Qi[QV][e] = s.ut; L.Qi[QP][e] = s.p;
    }
    __syncthreads();
    // F_x (fluxes.py:150-176, 189-221)
    for (int e = t; e < NFX; e += NT) {
        const int f = e / TJ, b = e % TJ;
        PrimN qa[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const int x = xf(f, b - 1 + r);
            qa[r] = PrimN{L.Qi[QR][x], L.Qi[QU][x], L.Qi[QV][x], L.Qi[QP][x]};
        }
        const double c24 = 1.0 / 24.0;
        PrimN fc;
        fc.r = qa[1].r - c24 * (qa[2].r - 2 * qa[1].r + qa[0].r);
        fc.un = qa[1].un - c24 * (qa[2].un - 2 * qa[1].un + qa[0].un);
        fc.ut = qa[1].ut - c24 * (qa[2].ut - 2 * qa[1].ut + qa[0].ut);
        fc.p = qa[1].p - c24 * (qa[2].p - 2 * qa[1].p + qa[0].p);
        double Ffc[4], Fa[3][4];
        flux_cons_n(fc, P.gamma, Ffc);
#pragma unroll
        for (int r = 0; r < 3; r++) flux_cons_n(qa[r], P.gamma, Fa[r]);
        // artificial viscosity, MC eqs. 35-36 (x: planes d, E, mx = mn, my = mt)
        const double *u = L.Qb[QU], *v = L.Qb[QV];
        const double lam = (u[B5::at(f, b)] - u[B5::at(f - 1, b)]) / P.dx +
                           0.25 * (v[B5::at(f, b + 1)] - v[B5::at(f, b - 1)] + v[B5::at(f - 1, b + 1)] -
                                   v[B5::at(f - 1, b - 1)]) / P.dy;
        const double dl = P.dx * lam;
        const double test = dl * dl / (0.3 * P.gamma * L.Qb[QP][B5::at(f, b)] / L.Qb[QR][B5::at(f, b)]);
        double nu = P.dx * lam * fmin(test, 1.0);
        if (lam >= 0.0) nu = 0.0;
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const double F = Ffc[n] + c24 * (Fa[2][n] - 2 * Fa[1][n] + Fa[0][n]);
            L.Fx[n][e] = F + 0.3 * nu * (L.U[n][B5::at(f, b)] - L.U[n][B5::at(f - 1, b)]);
        }
    }
    __syncthreads();

    // ---- 5. y faces ------------------------------------------------------------------------
    for (int e = t; e < (TI + 2) * (TJ + 1); e += NT) {
        const int a = e / (TJ + 1) - 1, gg = e % (TJ + 1);
        const int jg = j0 + gg;   // global index of the cell above the face
        const double xl = L.Xi[B1::at(a, gg - 1)], xr = L.Xi[B1::at(a, gg)];
        double ql[4], qr[4];
#pragma unroll
        for (int n = 0; n < 4; n++) {
            double w[8];
#pragma unroll
            for (int m = 0; m < 8; m++) w[m] = L.Qa[n][B4::at(a, gg - 4 + m)];
            double ar_l, al_f, ar_f, al_r;
            mc_limit(w, jg - 1 == g.jhi + 1, ar_l, al_f);
            mc_limit(w + 1, jg == g.jhi + 1, ar_f, al_r);
            ql[n] = xl * al_f + (1.0 - xl) * w[3];
            qr[n] = xr * ar_f + (1.0 - xr) * w[4];
        }
        const PrimN s = cgf_prim(PrimN{ql[QR], ql[QV], ql[QU], ql[QP]}, PrimN{qr[QR], qr[QV], qr[QU], qr[QP]},
                                 P.gamma);
        L.Qi[QR][e] = s.r; L.Qi[QU][e] = s.ut; L.Qi[QV][e] = s.un; L.Qi[QP][e] = s.p;
    }
    __syncthreads();
    for (int e = t; e < NFY; e += NT) {
        const int a = e / (TJ + 1), gg = e % (TJ + 1);
        PrimN qa[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const int x = yf(a - 1 + r, gg);
            qa[r] = PrimN{L.Qi[QR][x], L.Qi[QV][x], L.Qi[QU][x], L.Qi[QP][x]};
        }
        const double c24 = 1.0 / 24.0;
        PrimN fc;
        fc.r = qa[1].r - c24 * (qa[2].r - 2 * qa[1].r + qa[0].r);
        fc.un = qa[1].un - c24 * (qa[2].un - 2 * qa[1].un + qa[0].un);
        fc.ut = qa[1].ut - c24 * (qa[2].ut - 2 * qa[1].ut + qa[0].ut);
        fc.p = qa[1].p - c24 * (qa[2].p - 2 * qa[1].p + qa[0].p);
        double Ffc[4], Fa[3][4];
        flux_cons_n(fc, P.gamma, Ffc);
#pragma unroll
        for (int r = 0; r < 3; r++) flux_cons_n(qa[r], P.gamma, Fa[r]);
        const double *u = L.Qb[QU], *v = L.Qb[QV];
        const double lam = (v[B5::at(a, gg)] - v[B5::at(a, gg - 1)]) / P.dy +
                           0.25 * (u[B5::at(a + 1, gg)] - u[B5::at(a - 1, gg)] + u[B5::at(a + 1, gg - 1)] -
                                   u[B5::at(a - 1, gg - 1)]) / P.dx;
        const double dl = P.dx * lam;
        const double test = dl * dl / (0.3 * P.gamma * L.Qb[QP][B5::at(a, gg)] / L.Qb[QR][B5::at(a, gg)]);
        double nu = P.dx * lam * fmin(test, 1.0);
        if (lam >= 0.0) nu = 0.0;
        // (normal frame -> planes: mn is y-momentum, mt x-momentum)
        const int plane_of[4] = {0, 1, 3, 2};
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const int pn = plane_of[n];
            const double F = Ffc[n] + c24 * (Fa[2][n] - 2 * Fa[1][n] + Fa[0][n]);
            L.Fy[pn][e] = F + 0.3 * nu * (L.U[pn][B5::at(a, gg)] - L.U[pn][B5::at(a, gg - 1)]);
        }
    }
    __syncthreads();

    // ---- 6. k = -div F + <S> (- sponge), fv4/simulation.py:36-64 -----------------------------
    for (int e = t; e < TI * TJ; e += NT) {
        const int a = e / TJ, b = e % TJ;
        const int i = i0 + a, j = j0 + b;
        if (i > g.ihi || j > g.jhi) continue;
        const int c5 = B5::at(a, b);
        double Sv[4] = {0.0, 0.0, 0.0, 0.0};
        {
            const int c = B1::at(a, b), im = B1::at(a - 1, b), ip = B1::at(a + 1, b), jm = B1::at(a, b - 1),
                      jp = B1::at(a, b + 1);
            for (int n = 0; n < 2; n++) {
                const double *S = L.S[n];
                const double lap = (S[im] - 2 * S[c] + S[ip]) / dx2 + (S[jm] - 2 * S[c] + S[jp]) / dy2;
                Sv[n == 0 ? 1 : 3] = S[c] - dx2 * lap / 24.0;
            }
            // (the density and x-momentum sources are 0: 0 - dx^2 * 0 / 24)
            Sv[0] = 0.0 - dx2 * 0.0 / 24.0;
            Sv[2] = Sv[0];
        }
        double kk[4];
#pragma unroll
        for (int n = 0; n < 4; n++)
            kk[n] = (L.Fx[n][a * TJ + b] - L.Fx[n][(a + 1) * TJ + b]) / P.dx +
                    (L.Fy[n][a * (TJ + 1) + b] - L.Fy[n][a * (TJ + 1) + b + 1]) / P.dy + Sv[n];
        if (P.sponge) {
            const double PI = 3.14159265358979323846;
            const double d = L.U[0][c5], mx = L.U[2][c5], my = L.U[3][c5];
            double fs;
            if (d > P.rho_begin) fs = 0.0;
            else if (d < P.rho_full) fs = 1.0;
            else fs = 0.5 * (1.0 - cos(PI * (d - P.rho_begin) / (P.rho_full - P.rho_begin)));
            const double kap = fs / P.tau;
            kk[2] -= kap * mx;
            kk[3] -= kap * my;
            kk[1] -= kap * (mx * mx / d + my * my / d);
        }
        const size_t k = (size_t)i * g.pitch + j;
#pragma unroll
        for (int n = 0; n < 4; n++) K[n * pl + k] = kk[n];
    }
}

// The two launches of a right-hand side, nothing else: the flag is neither reset in front of them nor
// read back behind them.  S: the step scalars of a device-side run (pyrohip_comp_fv4_evolve /
// pyrohip_comp_sdc_evolve reset the flag once, at the open, and read it once, at the close); flag: the
// flag word of the call -- the state's own, or in a run the one of the state that is stepped, whichever
// stage or node state the right-hand side is taken of.
int comp_fv4_rhs_run(pyrohip_state *s, const pyrohip_comp_params *p, pyrohip_state *kst, int slot,
                     const StepScalars *S, int *flag)
{
    pyrohip_ctx *c = s->ctx;
    const Geom &g = s->g;
    FP P;
    P.gamma = p->gamma; P.dx = p->dx; P.dy = p->dy;
    P.z0 = p->z0; P.z1 = p->z1; P.delta = p->delta;
    P.small_dens = p->small_dens; P.grav = p->grav;
    P.heat = s->heat; P.heat_rate = s->heat ? p->heat_rate : 0.0;
    P.use_flattening = p->use_flattening;
    P.sponge = p->do_sponge;
    P.rho_begin = p->sponge_rho_begin; P.rho_full = p->sponge_rho_full; P.tau = p->sponge_timescale;
    PYRO_LAUNCH(c, "k_fv4_prep", k_fv4_prep, dim3((g.qy + 255) / 256, g.qx), dim3(256), 0, s->d, g, P,
                flag, S);
    PYRO_CHECK_HIP(hipGetLastError());   // (a refused prep launch must not be lost behind the next)
    const dim3 grid((g.nx + TI - 1) / TI, (g.ny + TJ - 1) / TJ);
    PYRO_LAUNCH(c, "k_fv4_rhs", k_fv4_rhs, grid, dim3(NT), 0, (const double *)s->d,
                kst->d + (size_t)(4 * slot) * g.plane, g, P, (const int *)flag);
    PYRO_CHECK_HIP(hipGetLastError());
    s->next_cfl_min = -1.0;
    return 0;
}

int comp_fv4_rhs(pyrohip_state *s, const pyrohip_comp_params *p, pyrohip_state *kst, int slot)
{
    pyrohip_ctx *c = s->ctx;
    PYRO_CHECK_HIP(hipMemsetAsync(s->d_flag, 0, sizeof(int), c->stream));
    PYRO_TRY(comp_fv4_rhs_run(s, p, kst, slot, nullptr, s->d_flag));
    PYRO_CHECK_HIP(hipMemcpyAsync(c->reduce_host, s->d_flag, sizeof(int), hipMemcpyDeviceToHost,
                                  c->stream));
    PYRO_CHECK_HIP(hipStreamSynchronize(c->stream));
    if (*(int *)c->reduce_host & 1) {
        set_error("invalid state: min(rho) <= 0 or min(e) <= 0 on the interior "
                  "(compressible/simulation.py:68-71, called by compressible_fv4/fluxes.py:80-81)");
        return PYROHIP_ERR_STATE;
    }
    return 0;
}

#if !PYRO_FAST
// fv.py:31-39: a <- a + dx^2 lap(a) / 24 on the interior, lap of the ghost-filled copy `src`
__global__ __launch_bounds__(256) void k_from_centers(double *__restrict__ a, const double *__restrict__ src,
                                                      Geom g, double dx, double dy)
{
    const int j = g.jlo + blockIdx.x * blockDim.x + threadIdx.x;
    const int i = g.ilo + blockIdx.y;
    if (j > g.jhi) return;
    const size_t k = (size_t)i * g.pitch + j;
    const double v = src[k];
    const double lap = (src[k - g.pitch] - 2 * v + src[k + g.pitch]) / (dx * dx) +
                       (src[k - 1] - 2 * v + src[k + 1]) / (dy * dy);
    a[k] = v + dx * dx * lap / 24.0;
}

int state_from_centers(pyrohip_state *s, int n, double dx, double dy, double *scratch)
{
    const Geom &g = s->g;
    double *a = s->d + (size_t)n * g.plane;
    PYRO_CHECK_HIP(hipMemcpyAsync(scratch, a, g.plane * sizeof(double), hipMemcpyDeviceToDevice,
                                  s->ctx->stream));
    PYRO_LAUNCH(s->ctx, "k_from_centers", k_from_centers, dim3((g.ny + 255) / 256, g.nx), dim3(256), 0, a,
                (const double *)scratch, g, dx, dy);
    PYRO_CHECK_HIP(hipGetLastError());
    return 0;
}

// compressible_sdc/simulation.py:85-87 with sdc_integral (:20-36):
// U[m+1] = U[m] + dt/2 (A_new[m] - A_old[m]) + dt/24 (c0 A_0 + c1 A_1 + c2 A_2), interior
struct SdcArgs { const double *an, *ao, *q0, *q1, *q2; double c0, c1, c2, hdt, idt; };
__global__ __launch_bounds__(256) void k_sdc_update(double *__restrict__ dst, const double *__restrict__ src,
                                                    Geom g, int nvar, SdcArgs A)
{
    const int j = g.jlo + blockIdx.x * blockDim.x + threadIdx.x;
    const int i = g.ilo + blockIdx.y;
    const int n = blockIdx.z;
    if (j > g.jhi || n >= nvar) return;
    const size_t k = (size_t)n * g.plane + (size_t)i * g.pitch + j;
    const double integral = A.idt * (A.c0 * A.q0[k] + A.c1 * A.q1[k] + A.c2 * A.q2[k]);
    dst[k] = src[k] + A.hdt * (A.an[k] - A.ao[k]) + integral;
}

int comp_sdc_update(pyrohip_state *dst, const pyrohip_state *src, const pyrohip_state *k, int slot_new,
                    int slot_old, const int *slots_q, const double *cq, double dt)
{
    const Geom &g = dst->g;
    const size_t blk = (size_t)dst->nvar * g.plane;
    SdcArgs A;
    A.an = k->d + slot_new * blk;
    A.ao = k->d + slot_old * blk;
    A.q0 = k->d + slots_q[0] * blk;
    A.q1 = k->d + slots_q[1] * blk;
    A.q2 = k->d + slots_q[2] * blk;
    A.c0 = cq[0]; A.c1 = cq[1]; A.c2 = cq[2];
    A.hdt = 0.5 * dt;
    A.idt = dt / 24.0;
    PYRO_LAUNCH(dst->ctx, "k_sdc_update", k_sdc_update, dim3((g.ny + 255) / 256, g.nx, dst->nvar), dim3(256),
                0, dst->d, (const double *)src->d, g, dst->nvar, A);
    PYRO_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the step of a device-side run (pyrohip_comp_fv4_evolve / pyrohip_comp_sdc_evolve) -------------
// Every state a right-hand side is taken of is formed AND ghost-filled by one launch: a thread per
// cell of the array evaluates the update at the cell's image under the composite x-then-y index map
// (array_indexer.py:163-274: x over all columns first, so a corner takes its value from an x ghost
// cell; what k_fill_frame2 does), with the sign of reflect-odd.  The launches read the start state and
// k and write another array, so a ghost cell never reads what another thread writes.  dt comes from
// the run's step scalars; an iteration that does not advance, or a raised flag, stores nothing.
struct Fv4Maps { BcMap mx[4], my[4]; };

static Fv4Maps fv4_maps(const pyrohip_state *s)
{
    const Geom &g = s->g;
    Fv4Maps M;
    for (int n = 0; n < 4; n++) {
        M.mx[n] = bc_map(g.ilo, g.ihi, g.ng, s->bc[n * 4 + 0], s->bc[n * 4 + 1], true);
        M.my[n] = bc_map(g.jlo, g.jhi, g.ng, s->bc[n * 4 + 2], s->bc[n * 4 + 3], true);
    }
    return M;
}

// the interior cell whose value array cell (i, j) of variable n shows; *neg: with the other sign
__device__ __forceinline__ size_t fv4_image(const Geom &g, const Fv4Maps &M, int n, int i, int j, bool *neg)
{
    const BcMap &mx = M.mx[n], &my = M.my[n];
    const int si = bc_src(mx, i, g.ilo, g.ihi), sj = bc_src(my, j, g.jlo, g.jhi);
    *neg = ((i < g.ilo && mx.odd_lo) || (i > g.ihi && mx.odd_hi)) !=
           ((j < g.jlo && my.odd_lo) || (j > g.jhi && my.odd_hi));
    return (size_t)si * g.pitch + sj;
}

__device__ __forceinline__ bool fv4_run_goes(const StepScalars *S, const int *flag)
{
    return S->active != 0 && *flag == 0;
}

// RKIntegrator.get_stage_start + the stage's ghost fill: dst = y + (dt c[0]) k_0 + (dt c[1]) k_1 + ...,
// k_lincomb's terms in its order (ctx.hip), each coefficient the once-rounded product dt * c[s] the
// host forms for pyrohip_state_lincomb; zero coefficients stay (0 * NaN is NaN)
struct Fv4Coef { double c[4]; int n; };
__global__ __launch_bounds__(256) void k_fv4_stage_start(double *__restrict__ dst, const double *__restrict__ y,
                                                         const double *__restrict__ K, Geom g, Fv4Maps M,
                                                         Fv4Coef lc, const StepScalars *__restrict__ S,
                                                         const int *__restrict__ flag)
{
    if (!fv4_run_goes(S, flag)) return;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y, n = blockIdx.z;
    if (j >= g.qy) return;
    bool neg;
    const size_t ks = fv4_image(g, M, n, i, j, &neg);
    const double dt = S->dt;
    double v = y[(size_t)n * g.plane + ks];
    for (int s = 0; s < lc.n; s++) {
        const double c = dt * lc.c[s];
        v += c * K[(size_t)(4 * s + n) * g.plane + ks];
    }
    dst[(size_t)n * g.plane + (size_t)i * g.pitch + j] = neg ? -v : v;
}

// compressible_rk/simulation.py:46-56 for one cell: k_rk_cfl's expression (compressible.hip)
__device__ __forceinline__ double fv4_cfl_cell(double d, double E, double mx, double my, double gamma, double dx,
                                               double dy)
{
    const double u = mx / d, v = my / d;
    const double e = (E - 0.5 * d * (u * u + v * v)) / d;
    const double pr = d * e * (gamma - 1.0);
    const double cs = sqrt(gamma * pr / d);
    return 1.0 / ((fabs(u) + cs) / dx + (fabs(v) + cs) / dy);
}

// RKIntegrator.compute_final_update (lc.n = nstages) or the copy of the last SDC node (lc.n = 0) into
// the state's OTHER buffer: the interior, and the ghost frame as the images of the new interior --
// what the next iteration's fill_BC_all would write.  An update in place could not write the frame: a
// ghost cell would read interior cells other threads overwrite.  One CFL partial per workgroup over
// the interior cells it wrote (with index-map ghost cells the interior's minimum is the array's).
__global__ __launch_bounds__(256) void k_fv4_final(double *__restrict__ dst, const double *__restrict__ y,
                                                   const double *__restrict__ K, Geom g, Fv4Maps M, Fv4Coef lc,
                                                   const StepScalars *__restrict__ S,
                                                   const int *__restrict__ flag, double gamma, double dx,
                                                   double dy, double *__restrict__ part)
{
    const int b = blockIdx.y * gridDim.x + blockIdx.x;
    if (!fv4_run_goes(S, flag)) {
        if (threadIdx.x == 0) part[b] = INFINITY;
        return;
    }
    const double dt = S->dt;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    double m = INFINITY;
    if (j < g.qy)
        for (int i = blockIdx.y; i < g.qx; i += gridDim.y) {
            double w[4];
#pragma unroll
            for (int n = 0; n < 4; n++) {
                bool neg;
                const size_t ks = fv4_image(g, M, n, i, j, &neg);
                double v = y[(size_t)n * g.plane + ks];
                for (int s = 0; s < lc.n; s++) {
                    const double c = dt * lc.c[s];
                    v += c * K[(size_t)(4 * s + n) * g.plane + ks];
                }
                w[n] = neg ? -v : v;
                dst[(size_t)n * g.plane + (size_t)i * g.pitch + j] = w[n];
            }
            if (i >= g.ilo && i <= g.ihi && j >= g.jlo && j <= g.jhi)
                m = fmin(m, fv4_cfl_cell(w[0], w[1], w[2], w[3], gamma, dx, dy));
        }
    m = block_reduce_min(m);
    if (threadIdx.x == 0) part[b] = m;
}

// k_sdc_update with the ghost fill of the destination node; hdt = dt / 2 and idt = dt / 24 from the
// run's dt, each rounded once as comp_sdc_update forms them on the host
__global__ __launch_bounds__(256) void k_fv4_sdc_node(double *__restrict__ dst, const double *__restrict__ src,
                                                      Geom g, Fv4Maps M, SdcArgs A,
                                                      const StepScalars *__restrict__ S,
                                                      const int *__restrict__ flag)
{
    if (!fv4_run_goes(S, flag)) return;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y, n = blockIdx.z;
    if (j >= g.qy) return;
    bool neg;
    const size_t k = (size_t)n * g.plane + fv4_image(g, M, n, i, j, &neg);
    const double dt = S->dt;
    const double hdt = 0.5 * dt, idt = dt / 24.0;
    const double integral = idt * (A.c0 * A.q0[k] + A.c1 * A.q1[k] + A.c2 * A.q2[k]);
    const double v = src[k] + hdt * (A.an[k] - A.ao[k]) + integral;
    dst[(size_t)n * g.plane + (size_t)i * g.pitch + j] = neg ? -v : v;
}

// ghost frame of the four planes src -> dst (the close of a run: the state handed back carries the
// filled ghost cells of the state before its last step, as after single steps)
__global__ __launch_bounds__(256) void k_fv4_copy_frame(double *__restrict__ dst, const double *__restrict__ src,
                                                        Geom g)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y, n = blockIdx.z;
    if (j >= g.qy || (i >= g.ilo && i <= g.ihi && j >= g.jlo && j <= g.jhi)) return;
    const size_t k = (size_t)n * g.plane + (size_t)i * g.pitch + j;
    dst[k] = src[k];
}

// stage state <- y + dt sum_j a[j] k_j (nterms terms, zeros included), ghost cells filled
int fv4_stage_start(pyrohip_state *stage, const pyrohip_state *y, const pyrohip_state *k, const double *a,
                    int nterms, const StepScalars *S)
{
    const Geom &g = y->g;
    Fv4Coef lc;
    lc.n = nterms;
    for (int s = 0; s < 4; s++) lc.c[s] = s < nterms ? a[s] : 0.0;
    PYRO_LAUNCH(y->ctx, "k_fv4_stage_start", k_fv4_stage_start, dim3((g.qy + 255) / 256, g.qx, 4), dim3(256), 0,
                stage->d, (const double *)y->d, (const double *)k->d, g, fv4_maps(y), lc, S,
                (const int *)y->d_flag);
    PYRO_CHECK_HIP(hipGetLastError());
    stage->next_cfl_min = -1.0;
    stage->ghost_by_rules = false;
    return 0;
}

// workgroups of k_fv4_final: pieces of 256 columns x at most 512 row slots (4608 partials at 2048^2)
int fv4_final_parts(const Geom &g) { return ((g.qy + 255) / 256) * (g.qx < 512 ? g.qx : 512); }

// the other buffer of y <- src + dt sum_s b[s] k_s (src: y itself, or the last SDC node with
// nterms = 0), ghost frame from the images, CFL partials into part; the buffers are NOT exchanged here
int fv4_final(pyrohip_state *y, const pyrohip_state *src, const pyrohip_state *k, const double *b, int nterms,
              const pyrohip_comp_params *p, const StepScalars *S, double *part)
{
    const Geom &g = y->g;
    Fv4Coef lc;
    lc.n = nterms;
    for (int s = 0; s < 4; s++) lc.c[s] = s < nterms ? b[s] : 0.0;
    const dim3 grid((g.qy + 255) / 256, g.qx < 512 ? g.qx : 512);
    PYRO_LAUNCH(y->ctx, "k_fv4_final", k_fv4_final, grid, dim3(256), 0, y->alt_base + geom_lead(g),
                (const double *)src->d, (const double *)k->d, g, fv4_maps(y), lc, S, (const int *)y->d_flag,
                p->gamma, p->dx, p->dy, part);
    PYRO_CHECK_HIP(hipGetLastError());
    return 0;
}

int fv4_sdc_node(pyrohip_state *dst, const pyrohip_state *src, const pyrohip_state *k, int slot_new,
                 int slot_old, const int *slots_q, const double *cq, const StepScalars *S, const int *flag)
{
    const Geom &g = dst->g;
    const size_t blk = (size_t)4 * g.plane;
    SdcArgs A;
    A.an = k->d + slot_new * blk;
    A.ao = k->d + slot_old * blk;
    A.q0 = k->d + slots_q[0] * blk;
    A.q1 = k->d + slots_q[1] * blk;
    A.q2 = k->d + slots_q[2] * blk;
    A.c0 = cq[0]; A.c1 = cq[1]; A.c2 = cq[2];
    A.hdt = 0.0; A.idt = 0.0;      // (formed by the kernel from the run's dt)
    PYRO_LAUNCH(dst->ctx, "k_fv4_sdc_node", k_fv4_sdc_node, dim3((g.qy + 255) / 256, g.qx, 4), dim3(256), 0,
                dst->d, (const double *)src->d, g, fv4_maps(dst), A, S, flag);
    PYRO_CHECK_HIP(hipGetLastError());
    dst->next_cfl_min = -1.0;
    dst->ghost_by_rules = false;
    return 0;
}

int fv4_copy_frame(pyrohip_state *dst, const double *src)
{
    const Geom &g = dst->g;
    PYRO_LAUNCH(dst->ctx, "k_fv4_copy_frame", k_fv4_copy_frame, dim3((g.qy + 255) / 256, g.qx, 4), dim3(256), 0,
                dst->d, src, g);
    PYRO_CHECK_HIP(hipGetLastError());
    return 0;
}
#endif

}  // namespace PYRO_NS
}  // namespace pyro
