// Low Mach number atmosphere (lm_atm): the pieces of Simulation.evolve between its two
// variable-coefficient multigrid solves, the time step and the coefficients of those solves.
//
//   pyro/lm_atm/simulation.py:138-178   method_compute_timestep
//   pyro/lm_atm/simulation.py:180-284   preevolve (initial projection)
//   pyro/lm_atm/simulation.py:286-618   evolve
//   pyro/lm_atm/LM_atm_interface.py     mac_vels, rho_states, states, riemann / upwind
//
// The state carries the solver's eight variables in the order the solver registers them
// (density, x-velocity, y-velocity, eint, phi-MAC, phi, gradp_x, gradp_y; ng = 4); the elliptic
// solves run in the pyrohip_mg (ng = 1) that is passed in.  The 1-d base state (rho0, p0, beta0
// and beta0 on the y edges, qy doubles each) lives behind the work planes of the state.
//
// Unlike incompressible.hip this unit computes on the reference's own ranges, the interior grown
// by 2 ("B2"): rho_states and states read MAC velocities on faces in the ghost region, which the
// MAC projection never corrects, and those are built from edge states of B2 cells that never see
// the transverse terms.  The limiter's "limit2 = 0 outside B2" rule therefore enters (lm_slope).
// Positions the reference never writes are read as 0 there (its scratch arrays) and here (the
// work area is zeroed once and every kernel writes the same set of positions every step).
// Compiled with -ffp-contract=off, reference operation order.
#include "common.h"
#include "mg_internal.h"
#include "reduce.h"
#include "stencil.h"

namespace pyro {

enum { LV_RHO, LV_U, LV_V, LV_EINT, LV_PHIMAC, LV_PHI, LV_GPX, LV_GPY, LV_NVAR };

// work planes
enum {
    H_UXL, H_UXR, H_UYL, H_UYR, H_VXL, H_VXR, H_VYL, H_VYR,   // normal-predictor ("hat") states
    T_UXL, T_UXR, T_UYL, T_UYR, T_VXL, T_VXR, T_VYL, T_VYR,   // + transverse, grad p, source on B1
    L_UMAC, L_VMAC, L_ADVX, L_ADVY,
    L_COEFF, L_SRC, L_RHOOLD,
    L_RXL, L_RXR, L_RYL, L_RYR, L_RXI, L_RYI,
    L_UXI, L_VXI, L_UYI, L_VYI,
    L_NPL
};

// LM_atm_interface.py:634-675
__device__ __forceinline__ double lm_riemann(double ql, double qr)
{
    if (ql > 0.0 && ql + qr > 0.0) return ql;
    if (ql <= 0.0 && qr >= 0.0) return 0.0;
    return qr;
}
// LM_atm_interface.py:588-629
__device__ __forceinline__ double lm_upwind(double ql, double qr, double s)
{
    if (s > 0.0) return ql;
    if (s == 0.0) return 0.5 * (ql + qr);
    return qr;
}

struct LP {   // kernel parameters
    double dx, dy, dt, dtdx, dtdy, grav, gamma;
    int limiter;
    const double *rho0, *p0, *beta0, *beta0e;   // 1-d base state (qy)
};

// reconstruction.limit at position `pos` of a line with interior [lo, hi]: limit2 is 0 outside
// the interior grown by 2, which limit4 sees in the cells on the rim of B2
__device__ __forceinline__ double lm_slope(const double *a, size_t k, int st, int pos, int lo,
                                           int hi, int limiter)
{
    const double am2 = a[k - 2 * st], am1 = a[k - st], a0 = a[k], ap1 = a[k + st],
                 ap2 = a[k + 2 * st];
    if (limiter < 2) return limited_slope(am2, am1, a0, ap1, ap2, limiter);
    const double l2p = (pos + 1 <= hi + 2) ? limit2(a0, ap1, ap2) : 0.0;
    const double l2m = (pos - 1 >= lo - 2) ? limit2(am2, am1, a0) : 0.0;
    return limit4_from(l2m, l2p, am1, a0, ap1);
}

// one thread per cell of B2
#define LM_CELL_B2()                                                   \
    const int j = g.jlo - 2 + blockIdx.x * blockDim.x + threadIdx.x;   \
    const int i = g.ilo - 2 + blockIdx.y;                              \
    if (j > g.jhi + 2) return;                                         \
    const int p = g.pitch;                                             \
    const size_t pl = g.plane;                                         \
    const size_t k = (size_t)i * p + j;
// one thread per face position of the reference's riemann / upwind range [lo - 1, hi + 2]^2
#define LM_FACE()                                                      \
    const int j = g.jlo - 1 + blockIdx.x * blockDim.x + threadIdx.x;   \
    const int i = g.ilo - 1 + blockIdx.y;                              \
    if (j > g.jhi + 2) return;                                         \
    const int p = g.pitch;                                             \
    const size_t pl = g.plane;                                         \
    const size_t k = (size_t)i * p + j;
// one thread per cell of the whole array / of the interior
#define LM_CELL_ALL()                                                  \
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y; \
    if (j >= g.qy) return;                                             \
    const int p = g.pitch;                                             \
    const size_t pl = g.plane;                                         \
    const size_t k = (size_t)i * p + j;                                \
    const bool in = (i >= g.ilo && i <= g.ihi && j >= g.jlo && j <= g.jhi);
#define LM_CELL_IN()                                                   \
    const int j = g.jlo + blockIdx.x * blockDim.x + threadIdx.x;       \
    const int i = g.ilo + blockIdx.y;                                  \
    if (j > g.jhi) return;                                             \
    const int p = g.pitch;                                             \
    const size_t pl = g.plane;                                         \
    const size_t k = (size_t)i * p + j;

// simulation.py:352-363: coeff = beta0 / rho and source = rho' g / rho on the interior
__global__ __launch_bounds__(256) void k_lm_coeff_src(const double *__restrict__ rho,
                                                      double *__restrict__ W, Geom g, LP P)
{
    LM_CELL_IN()
    (void)p;
    const double r = rho[k];
    double c = 1.0 / r;
    c = c * P.beta0[j];
    W[L_COEFF * pl + k] = c;
    W[L_SRC * pl + k] = (r - P.rho0[j]) * P.grav / r;
}

// get_interface_states, LM_atm_interface.py:487-518 (cells of B2)
__global__ __launch_bounds__(256) void k_lm_hat(const double *__restrict__ u,
                                                const double *__restrict__ v,
                                                double *__restrict__ W, Geom g, LP P)
{
    LM_CELL_B2()
    const double uc = u[k], vc = v[k];
    const double ldux = lm_slope(u, k, p, i, g.ilo, g.ihi, P.limiter);
    const double ldvx = lm_slope(v, k, p, i, g.ilo, g.ihi, P.limiter);
    const double lduy = lm_slope(u, k, 1, j, g.jlo, g.jhi, P.limiter);
    const double ldvy = lm_slope(v, k, 1, j, g.jlo, g.jhi, P.limiter);
    W[H_UXL * pl + k + p] = uc + 0.5 * (1.0 - P.dtdx * uc) * ldux;
    W[H_UXR * pl + k] = uc - 0.5 * (1.0 + P.dtdx * uc) * ldux;
    W[H_VXL * pl + k + p] = vc + 0.5 * (1.0 - P.dtdx * uc) * ldvx;
    W[H_VXR * pl + k] = vc - 0.5 * (1.0 + P.dtdx * uc) * ldvx;
    W[H_UYL * pl + k + 1] = uc + 0.5 * (1.0 - P.dtdy * vc) * lduy;
    W[H_UYR * pl + k] = uc - 0.5 * (1.0 + P.dtdy * vc) * lduy;
    W[H_VYL * pl + k + 1] = vc + 0.5 * (1.0 - P.dtdy * vc) * ldvy;
    W[H_VYR * pl + k] = vc - 0.5 * (1.0 + P.dtdy * vc) * ldvy;
}

// the transverse / grad p / source terms of get_interface_states (:544-581) for the states that
// belong to a cell of B1; the states of the other B2 cells stay as predicted (the reference
// updates its arrays in place)
__global__ __launch_bounds__(256) void k_lm_trans(const double *__restrict__ gpx,
                                                  const double *__restrict__ gpy,
                                                  double *__restrict__ W, Geom g, LP P)
{
    LM_CELL_B2()
    const double *uxl = W + H_UXL * pl, *uxr = W + H_UXR * pl, *uyl = W + H_UYL * pl,
                 *uyr = W + H_UYR * pl, *vxl = W + H_VXL * pl, *vxr = W + H_VXR * pl,
                 *vyl = W + H_VYL * pl, *vyr = W + H_VYR * pl;
    double a_uxl = uxl[k + p], a_uxr = uxr[k], a_vxl = vxl[k + p], a_vxr = vxr[k];
    double a_uyl = uyl[k + 1], a_uyr = uyr[k], a_vyl = vyl[k + 1], a_vyr = vyr[k];
    if (i >= g.ilo - 1 && i <= g.ihi + 1 && j >= g.jlo - 1 && j <= g.jhi + 1) {
        const double uh0 = lm_riemann(uxl[k], uxr[k]), uh1 = lm_riemann(uxl[k + p], uxr[k + p]);
        const double vh0 = lm_riemann(vyl[k], vyr[k]), vh1 = lm_riemann(vyl[k + 1], vyr[k + 1]);
        const double ubar = 0.5 * (uh0 + uh1), vbar = 0.5 * (vh0 + vh1);
        const double cf = W[L_COEFF * pl + k];
        const double gx = cf * gpx[k], gy = cf * gpy[k], src = W[L_SRC * pl + k];
        const double uy0 = lm_upwind(uyl[k], uyr[k], vh0), uy1 = lm_upwind(uyl[k + 1], uyr[k + 1], vh1);
        const double vy0 = lm_upwind(vyl[k], vyr[k], vh0), vy1 = lm_upwind(vyl[k + 1], vyr[k + 1], vh1);
        const double ux0 = lm_upwind(uxl[k], uxr[k], uh0), ux1 = lm_upwind(uxl[k + p], uxr[k + p], uh1);
        const double vx0 = lm_upwind(vxl[k], vxr[k], uh0), vx1 = lm_upwind(vxl[k + p], vxr[k + p], uh1);
        const double vu_y = vbar * (uy1 - uy0);
        a_uxl = a_uxl - 0.5 * P.dtdy * vu_y - 0.5 * P.dt * gx;
        a_uxr = a_uxr - 0.5 * P.dtdy * vu_y - 0.5 * P.dt * gx;
        const double vv_y = vbar * (vy1 - vy0);
        a_vxl = a_vxl - 0.5 * P.dtdy * vv_y - 0.5 * P.dt * gy + 0.5 * P.dt * src;
        a_vxr = a_vxr - 0.5 * P.dtdy * vv_y - 0.5 * P.dt * gy + 0.5 * P.dt * src;
        const double uv_x = ubar * (vx1 - vx0);
        a_vyl = a_vyl - 0.5 * P.dtdx * uv_x - 0.5 * P.dt * gy + 0.5 * P.dt * src;
        a_vyr = a_vyr - 0.5 * P.dtdx * uv_x - 0.5 * P.dt * gy + 0.5 * P.dt * src;
        const double uu_x = ubar * (ux1 - ux0);
        a_uyl = a_uyl - 0.5 * P.dtdx * uu_x - 0.5 * P.dt * gx;
        a_uyr = a_uyr - 0.5 * P.dtdx * uu_x - 0.5 * P.dt * gx;
    }
    W[T_UXL * pl + k + p] = a_uxl; W[T_UXR * pl + k] = a_uxr;
    W[T_VXL * pl + k + p] = a_vxl; W[T_VXR * pl + k] = a_vxr;
    W[T_UYL * pl + k + 1] = a_uyl; W[T_UYR * pl + k] = a_uyr;
    W[T_VYL * pl + k + 1] = a_vyl; W[T_VYR * pl + k] = a_vyr;
}

// riemann_and_upwind (:680-703) of the normal states
__global__ __launch_bounds__(256) void k_lm_mac(double *__restrict__ W, Geom g)
{
    LM_FACE()
    (void)p;
    {
        const double l = W[T_UXL * pl + k], r = W[T_UXR * pl + k];
        W[L_UMAC * pl + k] = lm_upwind(l, r, lm_riemann(l, r));
    }
    {
        const double l = W[T_VYL * pl + k], r = W[T_VYR * pl + k];
        W[L_VMAC * pl + k] = lm_upwind(l, r, lm_riemann(l, r));
    }
}

// simulation.py:408-411: div(beta0 U_MAC) into the finest multigrid level
__global__ __launch_bounds__(256) void k_lm_div_mac(const double *__restrict__ W, Geom g,
                                                    double *__restrict__ f, int mpitch, LP P)
{
    const int jj = blockIdx.x * blockDim.x + threadIdx.x, ii = blockIdx.y;
    if (jj >= g.ny) return;
    const int j = g.jlo + jj;
    const size_t k = (size_t)(g.ilo + ii) * g.pitch + j;
    const double *um = W + L_UMAC * g.plane, *vm = W + L_VMAC * g.plane;
    f[(size_t)(ii + 1) * mpitch + jj + 1] =
        P.beta0[j] * (um[k + g.pitch] - um[k]) / P.dx +
        (P.beta0e[j + 1] * vm[k + 1] - P.beta0e[j] * vm[k]) / P.dy;
}

// eta = beta0^2 / rho on the finest multigrid level (simulation.py:389-390, :552-553, :205-207).
// Written on the interior grown by one; the ghost fill that follows replaces the ghost values.
__global__ __launch_bounds__(256) void k_lm_eta(const double *__restrict__ rho, Geom g,
                                                double *__restrict__ c, int mpitch, LP P)
{
    const int jj = blockIdx.x * blockDim.x + threadIdx.x, ii = blockIdx.y;   // MG indices
    if (jj > g.ny + 1) return;
    const int j = g.jlo + jj - 1;
    const size_t k = (size_t)(g.ilo + ii - 1) * g.pitch + j;
    const double b = P.beta0[j];
    double e = 1.0 / rho[k];
    e = e * (b * b);
    c[(size_t)ii * mpitch + jj] = e;
}

// solution on B1, zero elsewhere (MG.get_solution(grid=myg), MG.py:414-437)
__global__ __launch_bounds__(256) void k_lm_copy_b1(const double *__restrict__ mv, int mpitch,
                                                    double *__restrict__ dst, Geom g)
{
    LM_CELL_ALL()
    (void)pl; (void)in;
    const bool b1 = (i >= g.ilo - 1 && i <= g.ihi + 1 && j >= g.jlo - 1 && j <= g.jhi + 1);
    dst[k] = b1 ? mv[(size_t)(i - g.ilo + 1) * mpitch + (j - g.jlo + 1)] : 0.0;
}

// MAC correction with the face-averaged beta0 / rho (simulation.py:428-444): u on the x faces
// [ilo, ihi + 1] of the interior rows, v on the y faces [jlo, jhi + 1] of the interior columns
__global__ __launch_bounds__(256) void k_lm_mac_project(double *__restrict__ W,
                                                        const double *__restrict__ phiM, Geom g,
                                                        LP P)
{
    const int j = g.jlo + blockIdx.x * blockDim.x + threadIdx.x;
    const int i = g.ilo + blockIdx.y;
    if (j > g.jhi + 1) return;
    const int p = g.pitch;
    const size_t pl = g.plane;
    const size_t k = (size_t)i * p + j;
    const double *cf = W + L_COEFF * pl;
    if (j <= g.jhi) {
        const double cx = 0.5 * (cf[k - p] + cf[k]);
        W[L_UMAC * pl + k] -= cx * (phiM[k] - phiM[k - p]) / P.dx;
    }
    if (i <= g.ihi) {
        const double cy = 0.5 * (cf[k - 1] + cf[k]);
        W[L_VMAC * pl + k] -= cy * (phiM[k] - phiM[k - 1]) / P.dy;
    }
}

// rho_states (LM_atm_interface.py:375-388): normal predictor of rho with the MAC velocities
__global__ __launch_bounds__(256) void k_lm_rho_hat(const double *__restrict__ rho,
                                                    double *__restrict__ W, Geom g, LP P)
{
    LM_CELL_B2()
    const double *um = W + L_UMAC * pl, *vm = W + L_VMAC * pl;
    const double r = rho[k];
    const double ldrx = lm_slope(rho, k, p, i, g.ilo, g.ihi, P.limiter);
    const double ldry = lm_slope(rho, k, 1, j, g.jlo, g.jhi, P.limiter);
    W[L_RXL * pl + k + p] = r + 0.5 * (1.0 - P.dtdx * um[k + p]) * ldrx;
    W[L_RXR * pl + k] = r - 0.5 * (1.0 + P.dtdx * um[k]) * ldrx;
    W[L_RYL * pl + k + 1] = r + 0.5 * (1.0 - P.dtdy * vm[k + 1]) * ldry;
    W[L_RYR * pl + k] = r - 0.5 * (1.0 + P.dtdy * vm[k]) * ldry;
}

// upwind(rho_xl, rho_xr, u_MAC), upwind(rho_yl, rho_yr, v_MAC)  (:391-392 and :421-422)
__global__ __launch_bounds__(256) void k_lm_rho_int(double *__restrict__ W, Geom g)
{
    LM_FACE()
    (void)p;
    W[L_RXI * pl + k] = lm_upwind(W[L_RXL * pl + k], W[L_RXR * pl + k], W[L_UMAC * pl + k]);
    W[L_RYI * pl + k] = lm_upwind(W[L_RYL * pl + k], W[L_RYR * pl + k], W[L_VMAC * pl + k]);
}

// transverse term and non-advective part of the normal divergence (:396-418)
__global__ __launch_bounds__(256) void k_lm_rho_trans(const double *__restrict__ rho,
                                                      double *__restrict__ W, Geom g, LP P)
{
    LM_CELL_B2()
    const double *um = W + L_UMAC * pl, *vm = W + L_VMAC * pl;
    const double *rxi = W + L_RXI * pl, *ryi = W + L_RYI * pl;
    const double r = rho[k];
    const double u_x = (um[k + p] - um[k]) / P.dx;
    const double v_y = (vm[k + 1] - vm[k]) / P.dy;
    const double rhov_y = (ryi[k + 1] * vm[k + 1] - ryi[k] * vm[k]) / P.dy;
    const double rhou_x = (rxi[k + p] * um[k + p] - rxi[k] * um[k]) / P.dx;
    const double tx = 0.5 * P.dt * (rhov_y + r * u_x);
    const double ty = 0.5 * P.dt * (rhou_x + r * v_y);
    W[L_RXL * pl + k + p] = W[L_RXL * pl + k + p] - tx;
    W[L_RXR * pl + k] = W[L_RXR * pl + k] - tx;
    W[L_RYL * pl + k + 1] = W[L_RYL * pl + k + 1] - ty;
    W[L_RYR * pl + k] = W[L_RYR * pl + k] - ty;
}

// rho_old = rho.copy() and the conservative update of the interior (simulation.py:456-462)
__global__ __launch_bounds__(256) void k_lm_rho_update(double *__restrict__ rho,
                                                       double *__restrict__ W, Geom g, LP P)
{
    LM_CELL_ALL()
    const double r = rho[k];
    W[L_RHOOLD * pl + k] = r;
    if (!in) return;
    const double *um = W + L_UMAC * pl, *vm = W + L_VMAC * pl;
    const double *rxi = W + L_RXI * pl, *ryi = W + L_RYI * pl;
    rho[k] = r - P.dt * ((rxi[k + p] * um[k + p] - rxi[k] * um[k]) / P.dx +
                         (ryi[k + 1] * vm[k + 1] - ryi[k] * vm[k]) / P.dy);
}

// eint (:467-469) and coeff = 2 beta0 / (rho + rho_old) (:478-480) on the interior
__global__ __launch_bounds__(256) void k_lm_eint_coeff(const double *__restrict__ rho,
                                                       double *__restrict__ eint,
                                                       double *__restrict__ W, Geom g, LP P)
{
    LM_CELL_IN()
    (void)p;
    const double r = rho[k];
    eint[k] = P.p0[j] / (P.gamma - 1.0) / r;
    double c = 2.0 / (r + W[L_RHOOLD * pl + k]);
    c = c * P.beta0[j];
    W[L_COEFF * pl + k] = c;
}

// states (:320-325): upwind the full states with the MAC velocities
__global__ __launch_bounds__(256) void k_lm_vel_int(double *__restrict__ W, Geom g)
{
    LM_FACE()
    (void)p;
    const double um = W[L_UMAC * pl + k], vm = W[L_VMAC * pl + k];
    W[L_UXI * pl + k] = lm_upwind(W[T_UXL * pl + k], W[T_UXR * pl + k], um);
    W[L_VXI * pl + k] = lm_upwind(W[T_VXL * pl + k], W[T_VXR * pl + k], um);
    W[L_UYI * pl + k] = lm_upwind(W[T_UYL * pl + k], W[T_UYR * pl + k], vm);
    W[L_VYI * pl + k] = lm_upwind(W[T_VYL * pl + k], W[T_VYR * pl + k], vm);
}

// advective terms and provisional update (simulation.py:506-525)
__global__ __launch_bounds__(256) void k_lm_advect(double *__restrict__ u, double *__restrict__ v,
                                                   const double *__restrict__ gpx,
                                                   const double *__restrict__ gpy,
                                                   double *__restrict__ W, Geom g, LP P,
                                                   int proj_type)
{
    LM_CELL_IN()
    const double *um = W + L_UMAC * pl, *vm = W + L_VMAC * pl;
    const double *uxi = W + L_UXI * pl, *vxi = W + L_VXI * pl, *uyi = W + L_UYI * pl,
                 *vyi = W + L_VYI * pl;
    const double ub = 0.5 * (um[k] + um[k + p]), vb = 0.5 * (vm[k] + vm[k + 1]);
    const double ax = ub * (uxi[k + p] - uxi[k]) / P.dx + vb * (uyi[k + 1] - uyi[k]) / P.dy;
    const double ay = ub * (vxi[k + p] - vxi[k]) / P.dx + vb * (vyi[k + 1] - vyi[k]) / P.dy;
    W[L_ADVX * pl + k] = ax;
    W[L_ADVY * pl + k] = ay;
    if (proj_type == 1) {
        u[k] -= (P.dt * ax + P.dt * gpx[k]);
        v[k] -= (P.dt * ay + P.dt * gpy[k]);
    } else {
        u[k] -= P.dt * ax;
        v[k] -= P.dt * ay;
    }
}

// buoyancy from rho_half over the whole array (simulation.py:528-530)
__global__ __launch_bounds__(256) void k_lm_buoy(const double *__restrict__ rho,
                                                 double *__restrict__ W, Geom g, LP P)
{
    LM_CELL_ALL()
    (void)p; (void)in;
    const double rh = 0.5 * (rho[k] + W[L_RHOOLD * pl + k]);
    W[L_SRC * pl + k] = (rh - P.rho0[j]) * P.grav / rh;
}
// v[:, :] += dt * source (:533)
__global__ __launch_bounds__(256) void k_lm_add_src(double *__restrict__ v,
                                                    const double *__restrict__ W, Geom g, LP P)
{
    LM_CELL_ALL()
    (void)p; (void)in;
    v[k] += P.dt * W[L_SRC * pl + k];
}

// cell-centred div(beta0 U) [/ dt] -> f (simulation.py:570-574, :226-228); guess = phi on B1
// (:577-579) or zeros
__global__ __launch_bounds__(256) void k_lm_div_cc(const double *__restrict__ u,
                                                   const double *__restrict__ v,
                                                   const double *__restrict__ phi, Geom g,
                                                   double *__restrict__ f, double *__restrict__ mv,
                                                   int mpitch, LP P, int divide_by_dt)
{
    const int jj = blockIdx.x * blockDim.x + threadIdx.x, ii = blockIdx.y;   // MG indices
    if (jj > g.ny + 1) return;
    const size_t mk = (size_t)ii * mpitch + jj;
    const int j = g.jlo + jj - 1;
    const size_t k = (size_t)(g.ilo + ii - 1) * g.pitch + j;
    mv[mk] = phi ? phi[k] : 0.0;
    if (ii >= 1 && ii <= g.nx && jj >= 1 && jj <= g.ny) {
        double d = 0.5 * P.beta0[j] * (u[k + g.pitch] - u[k - g.pitch]) / P.dx +
                   0.5 * (P.beta0[j + 1] * v[k + 1] - P.beta0[j - 1] * v[k - 1]) / P.dy;
        if (divide_by_dt) d = d / P.dt;
        f[mk] = d;
    }
}

// solution gradient (MG.py:439-469), U -= fac (beta0 / rho) grad(phi), grad p rule
// (simulation.py:590-607; :245-251 with fac = 1 and gp_mode 0)
__global__ __launch_bounds__(256) void k_lm_proj_update(const double *__restrict__ rho,
                                                        double *__restrict__ u,
                                                        double *__restrict__ v,
                                                        double *__restrict__ gpx,
                                                        double *__restrict__ gpy,
                                                        const double *__restrict__ mv, int mpitch,
                                                        Geom g, LP P, double fac, int gp_mode)
{
    LM_CELL_IN()
    (void)p; (void)pl;
    const size_t mk = (size_t)(i - g.ilo + 1) * mpitch + (j - g.jlo + 1);
    const double gx = 0.5 * (mv[mk + mpitch] - mv[mk - mpitch]) / P.dx;
    const double gy = 0.5 * (mv[mk + 1] - mv[mk - 1]) / P.dy;
    double c = 1.0 / rho[k];
    c = c * P.beta0[j];
    u[k] -= fac * c * gx;
    v[k] -= fac * c * gy;
    if (gp_mode == 1) { gpx[k] += gx; gpy[k] += gy; }
    else if (gp_mode == 2) { gpx[k] = gx; gpy[k] = gy; }
}

// method_compute_timestep (simulation.py:138-178): per-workgroup maxima of |u|, |v| over the
// interior and over the whole array and of |rho' g| / rho over the interior ...
__global__ __launch_bounds__(256) void k_lm_dt_partial(const double *__restrict__ rho,
                                                       const double *__restrict__ u,
                                                       const double *__restrict__ v, Geom g, LP P,
                                                       double *__restrict__ part)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    double ui = 0.0, vi = 0.0, ua = 0.0, va = 0.0, fb = 0.0;
    if (j < g.qy) {
        const size_t k = (size_t)i * g.pitch + j;
        ua = fabs(u[k]);
        va = fabs(v[k]);
        if (i >= g.ilo && i <= g.ihi && j >= g.jlo && j <= g.jhi) {
            ui = ua;
            vi = va;
            const double r = rho[k];
            fb = fabs((r - P.rho0[j]) * P.grav) / r;
        }
    }
    ui = block_reduce_max(ui);
    vi = block_reduce_max(vi);
    ua = block_reduce_max(ua);
    va = block_reduce_max(va);
    fb = block_reduce_max(fb);
    if (threadIdx.x == 0) {
        double *o = part + 5 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        o[0] = ui; o[1] = vi; o[2] = ua; o[3] = va; o[4] = fb;
    }
}
// ... and the time step from them: out = dt, max|u|, max|v| (interior), max|u|, max|v| (whole
// array), F_buoy
__global__ __launch_bounds__(256) void k_lm_dt_final(const double *__restrict__ part, int nb,
                                                     double dx, double dy, double cfl,
                                                     double *__restrict__ out)
{
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nb; b += blockDim.x)
        for (int q = 0; q < 5; q++) m[q] = fmax(m[q], part[5 * (size_t)b + q]);
    for (int q = 0; q < 5; q++) m[q] = block_reduce_max(m[q]);
    if (threadIdx.x == 0) {
        double xtmp = 1.e33, ytmp = 1.e33;
        if (!(m[2] == 0.0)) xtmp = dx / m[0];
        if (!(m[3] == 0.0)) ytmp = dy / m[1];
        double dt = cfl * fmin(xtmp, ytmp);
        const double dt_buoy = sqrt(2.0 * dx / m[4]);
        dt = fmin(dt, dt_buoy);
        out[0] = dt;
        for (int q = 0; q < 5; q++) out[1 + q] = m[q];
    }
}

static size_t lm_base_stride(const Geom &g) { return (size_t)((g.qy + 15) / 16) * 16; }

static LP make_lp(const pyrohip_state *s, double dx, double dy, double dt, int limiter,
                  double grav, double gamma)
{
    LP P;
    P.dx = dx; P.dy = dy; P.dt = dt; P.dtdx = dt / dx; P.dtdy = dt / dy;
    P.grav = grav; P.gamma = gamma; P.limiter = limiter;
    const double *b = s->work + s->g.plane * L_NPL + 16;
    const size_t st = lm_base_stride(s->g);
    P.rho0 = b; P.p0 = b + st; P.beta0 = b + 2 * st; P.beta0e = b + 3 * st;
    return P;
}

// ghost fill of one work plane with the boundary types of state variable n
static int lm_fill_work(pyrohip_state *s, int plane, int n)
{
    double *w = s->work + geom_lead(s->g) + (size_t)plane * s->g.plane;
    return fill_bc_planes(s, w - (size_t)n * s->g.plane, n, 1);
}

// the second half of get_interface_states with the current coeff / source planes
static void lm_trans(pyrohip_state *s, const LP &P)
{
    const Geom &g = s->g;
    PYRO_LAUNCH(s->ctx, "k_lm_trans", k_lm_trans, dim3((g.ny + 4 + 255) / 256, g.nx + 4), dim3(256),
                0, (const double *)(s->d + (size_t)LV_GPX * g.plane),
                (const double *)(s->d + (size_t)LV_GPY * g.plane), s->work + geom_lead(g), g, P);
}

}  // namespace pyro

using namespace pyro;

#define LM_CHECK_STATE(s)                                                                      \
    PYRO_REQUIRE((s), "NULL state");                                                           \
    PYRO_REQUIRE((s)->nvar == LV_NVAR && (s)->g.ng >= 4,                                       \
                 "lm_atm needs the solver's eight variables and ng >= 4");                     \
    PYRO_REQUIRE(state_work_is((s), WorkOwner::LM, L_NPL), "call pyrohip_lm_set_base first")
#define LM_CHECK_MG(s, m, F)                                                                   \
    LM_CHECK_STATE(s);                                                                         \
    PYRO_REQUIRE((m), "NULL mg");                                                              \
    MgFinest F;                                                                                \
    PYRO_TRY(mg_finest((m), &F));                                                              \
    PYRO_REQUIRE(F.ctx == (s)->ctx, "state and multigrid live on different contexts");         \
    PYRO_REQUIRE((s)->g.nx == F.n && (s)->g.ny == F.n, "state and multigrid sizes differ")

extern "C" {

int pyrohip_lm_set_base(pyrohip_state *s, const double *rho0, const double *p0,
                        const double *beta0, const double *beta0_edges)
{
    PYRO_REQUIRE(s && rho0 && p0 && beta0 && beta0_edges, "NULL argument");
    PYRO_REQUIRE(s->nvar == LV_NVAR && s->g.ng >= 4,
                 "lm_atm needs the solver's eight variables and ng >= 4");
    // work planes + the four base-state arrays behind them; owner LM = the base state is set
    PYRO_TRY(state_work(s, WorkOwner::LM, L_NPL, 4 * lm_base_stride(s->g)));
    const LP P = make_lp(s, 1.0, 1.0, 0.0, 0, 0.0, 0.0);
    const size_t nb = (size_t)s->g.qy * sizeof(double);
    hipStream_t st = s->ctx->stream;
    PYRO_CHECK_HIP(hipMemcpyAsync((void *)P.rho0, rho0, nb, hipMemcpyHostToDevice, st));
    PYRO_CHECK_HIP(hipMemcpyAsync((void *)P.p0, p0, nb, hipMemcpyHostToDevice, st));
    PYRO_CHECK_HIP(hipMemcpyAsync((void *)P.beta0, beta0, nb, hipMemcpyHostToDevice, st));
    PYRO_CHECK_HIP(hipMemcpyAsync((void *)P.beta0e, beta0_edges, nb, hipMemcpyHostToDevice, st));
    PYRO_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

int pyrohip_lm_dt(pyrohip_state *s, double dx, double dy, double cfl, double grav, double *out6)
{
    LM_CHECK_STATE(s);
    PYRO_REQUIRE(out6, "NULL argument");
    pyrohip_ctx *c = s->ctx;
    const Geom &g = s->g;
    const LP P = make_lp(s, dx, dy, 0.0, 0, grav, 0.0);
    const dim3 grid((g.qy + 255) / 256, g.qx);
    const int nb = (int)(grid.x * grid.y);
    PYRO_TRY(c->reduce.ensure(((size_t)5 * nb + 8) * sizeof(double)));
    double *part = (double *)c->reduce.p, *res = part + (size_t)5 * nb;
    PYRO_LAUNCH(c, "k_lm_dt_partial", k_lm_dt_partial, grid, dim3(256), 0,
                (const double *)(s->d + (size_t)LV_RHO * g.plane),
                (const double *)(s->d + (size_t)LV_U * g.plane),
                (const double *)(s->d + (size_t)LV_V * g.plane), g, P, part);
    PYRO_LAUNCH(c, "k_lm_dt_final", k_lm_dt_final, dim3(1), dim3(256), 0, (const double *)part, nb,
                dx, dy, cfl, res);
    PYRO_CHECK_HIP(hipGetLastError());
    PYRO_CHECK_HIP(hipMemcpyAsync(out6, res, 6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PYRO_CHECK_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int pyrohip_lm_mg_coeffs(pyrohip_state *s, pyrohip_mg *m)
{
    LM_CHECK_MG(s, m, F);
    const Geom &g = s->g;
    const LP P = make_lp(s, 1.0, 1.0, 0.0, 0, 0.0, 0.0);
    double *fc = nullptr;
    int fpitch = 0;
    PYRO_TRY(mg_coeffs_begin(m, &fc, &fpitch));
    PYRO_LAUNCH(s->ctx, "k_lm_eta", k_lm_eta, dim3((g.ny + 2 + 255) / 256, g.nx + 2), dim3(256), 0,
                (const double *)(s->d + (size_t)LV_RHO * g.plane), g, fc, fpitch, P);
    return mg_coeffs_finish(m, s->bc.data() + 4 * LV_RHO);   // coeffs_bc = the density's
}

int pyrohip_lm_mac_rhs(pyrohip_state *s, pyrohip_mg *m, double dx, double dy, double dt,
                       int limiter, double grav, double *source_norm)
{
    LM_CHECK_MG(s, m, F);
    pyrohip_ctx *c = s->ctx;
    const Geom &g = s->g;
    const LP P = make_lp(s, dx, dy, dt, limiter, grav, 0.0);
    double *W = s->work + geom_lead(g);
    const double *rho = s->d + (size_t)LV_RHO * g.plane, *u = s->d + (size_t)LV_U * g.plane,
                 *v = s->d + (size_t)LV_V * g.plane;
    const dim3 block(256), gridI((g.ny + 255) / 256, g.nx), gridB2((g.ny + 4 + 255) / 256, g.nx + 4),
        gridF((g.ny + 3 + 255) / 256, g.nx + 3);
    PYRO_LAUNCH(c, "k_lm_coeff_src", k_lm_coeff_src, gridI, block, 0, rho, W, g, P);
    PYRO_TRY(lm_fill_work(s, L_COEFF, LV_RHO));
    PYRO_TRY(lm_fill_work(s, L_SRC, LV_V));
    PYRO_LAUNCH(c, "k_lm_hat", k_lm_hat, gridB2, block, 0, u, v, W, g, P);
    lm_trans(s, P);
    PYRO_LAUNCH(c, "k_lm_mac", k_lm_mac, gridF, block, 0, W, g);
    PYRO_TRY(pyrohip_mg_zero(m, F.level, 0));   // a fresh multigrid object: v = 0
    PYRO_TRY(pyrohip_mg_zero(m, F.level, 1));
    PYRO_LAUNCH(c, "k_lm_div_mac", k_lm_div_mac, gridI, block, 0, (const double *)W, g, F.f,
                F.pitch, P);
    PYRO_CHECK_HIP(hipGetLastError());
    return pyrohip_mg_init_rhs_norm(m, source_norm);
}

int pyrohip_lm_advect(pyrohip_state *s, pyrohip_mg *m, double dx, double dy, double dt,
                      int limiter, int proj_type, double grav, double gamma)
{
    LM_CHECK_MG(s, m, F);
    PYRO_REQUIRE(proj_type == 1 || proj_type == 2, "proj_type must be 1 or 2");
    pyrohip_ctx *c = s->ctx;
    const Geom &g = s->g;
    const LP P = make_lp(s, dx, dy, dt, limiter, grav, gamma);
    double *W = s->work + geom_lead(g);
    double *rho = s->d + (size_t)LV_RHO * g.plane, *u = s->d + (size_t)LV_U * g.plane,
           *v = s->d + (size_t)LV_V * g.plane, *phiM = s->d + (size_t)LV_PHIMAC * g.plane;
    const dim3 block(256), gridI((g.ny + 255) / 256, g.nx), gridA((g.qy + 255) / 256, g.qx),
        gridB2((g.ny + 4 + 255) / 256, g.nx + 4), gridF((g.ny + 3 + 255) / 256, g.nx + 3);
    PYRO_TRY(mg_solution_ghosts(m));   // solve() ends with fill_BC(v)
    PYRO_LAUNCH(c, "k_lm_copy_b1", k_lm_copy_b1, gridA, block, 0, (const double *)F.v, F.pitch,
                phiM, g);
    // the reference recomputes coeff = beta0 / rho here (:423-426): rho has not changed since
    // pyrohip_lm_mac_rhs, the coeff and source planes still hold exactly those values
    PYRO_LAUNCH(c, "k_lm_mac_project", k_lm_mac_project, dim3((g.ny + 1 + 255) / 256, g.nx + 1),
                block, 0, W, (const double *)phiM, g, P);
    PYRO_LAUNCH(c, "k_lm_rho_hat", k_lm_rho_hat, gridB2, block, 0, (const double *)rho, W, g, P);
    PYRO_LAUNCH(c, "k_lm_rho_int", k_lm_rho_int, gridF, block, 0, W, g);
    PYRO_LAUNCH(c, "k_lm_rho_trans", k_lm_rho_trans, gridB2, block, 0, (const double *)rho, W, g, P);
    PYRO_LAUNCH(c, "k_lm_rho_int", k_lm_rho_int, gridF, block, 0, W, g);
    PYRO_LAUNCH(c, "k_lm_rho_update", k_lm_rho_update, gridA, block, 0, rho, W, g, P);
    PYRO_TRY(fill_bc_planes(s, s->d, LV_RHO, 1));
    PYRO_LAUNCH(c, "k_lm_eint_coeff", k_lm_eint_coeff, gridI, block, 0, (const double *)rho,
                s->d + (size_t)LV_EINT * g.plane, W, g, P);
    PYRO_TRY(lm_fill_work(s, L_COEFF, LV_RHO));
    lm_trans(s, P);
    PYRO_LAUNCH(c, "k_lm_vel_int", k_lm_vel_int, gridF, block, 0, W, g);
    PYRO_LAUNCH(c, "k_lm_advect", k_lm_advect, gridI, block, 0, u, v,
                (const double *)(s->d + (size_t)LV_GPX * g.plane),
                (const double *)(s->d + (size_t)LV_GPY * g.plane), W, g, P, proj_type);
    PYRO_LAUNCH(c, "k_lm_buoy", k_lm_buoy, gridA, block, 0, (const double *)rho, W, g, P);
    PYRO_TRY(lm_fill_work(s, L_SRC, LV_V));
    PYRO_LAUNCH(c, "k_lm_add_src", k_lm_add_src, gridA, block, 0, v, (const double *)W, g, P);
    PYRO_TRY(fill_bc_planes(s, s->d, LV_U, 2));
    PYRO_CHECK_HIP(hipGetLastError());
    s->next_cfl_min = -1.0;
    s->ghost_by_rules = false;
    return 0;
}

int pyrohip_lm_proj_rhs(pyrohip_state *s, pyrohip_mg *m, double dx, double dy, double dt,
                        int divide_by_dt, int use_guess, double *source_norm)
{
    LM_CHECK_MG(s, m, F);
    const Geom &g = s->g;
    const LP P = make_lp(s, dx, dy, dt, 0, 0.0, 0.0);
    PYRO_TRY(pyrohip_mg_zero(m, F.level, 1));
    PYRO_LAUNCH(s->ctx, "k_lm_div_cc", k_lm_div_cc, dim3((g.ny + 2 + 255) / 256, g.nx + 2),
                dim3(256), 0, (const double *)(s->d + (size_t)LV_U * g.plane),
                (const double *)(s->d + (size_t)LV_V * g.plane),
                use_guess ? (const double *)(s->d + (size_t)LV_PHI * g.plane) : nullptr, g, F.f,
                F.v, F.pitch, P, divide_by_dt);
    PYRO_CHECK_HIP(hipGetLastError());
    PYRO_TRY(mg_solution_written(m));
    return pyrohip_mg_init_rhs_norm(m, source_norm);
}

int pyrohip_lm_proj_update(pyrohip_state *s, pyrohip_mg *m, double dx, double dy, double fac,
                           int gp_mode)
{
    LM_CHECK_MG(s, m, F);
    PYRO_REQUIRE(gp_mode >= 0 && gp_mode <= 2, "gp_mode: 0 none, 1 +=, 2 =");
    pyrohip_ctx *c = s->ctx;
    const Geom &g = s->g;
    const LP P = make_lp(s, dx, dy, 0.0, 0, 0.0, 0.0);
    const dim3 block(256);
    PYRO_TRY(mg_solution_ghosts(m));   // solve() ends with fill_BC(v)
    PYRO_LAUNCH(c, "k_lm_copy_b1", k_lm_copy_b1, dim3((g.qy + 255) / 256, g.qx), block, 0,
                (const double *)F.v, F.pitch, s->d + (size_t)LV_PHI * g.plane, g);
    PYRO_LAUNCH(c, "k_lm_proj_update", k_lm_proj_update, dim3((g.ny + 255) / 256, g.nx), block, 0,
                (const double *)(s->d + (size_t)LV_RHO * g.plane), s->d + (size_t)LV_U * g.plane,
                s->d + (size_t)LV_V * g.plane, s->d + (size_t)LV_GPX * g.plane,
                s->d + (size_t)LV_GPY * g.plane, (const double *)F.v, F.pitch, g, P, fac, gp_mode);
    PYRO_TRY(fill_bc_planes(s, s->d, LV_U, 2));
    if (gp_mode) PYRO_TRY(fill_bc_planes(s, s->d, LV_GPX, 2));
    PYRO_CHECK_HIP(hipGetLastError());
    s->next_cfl_min = -1.0;
    s->ghost_by_rules = false;
    return 0;
}

// which: 0-7 full edge states (u_xl u_xr u_yl u_yr v_xl v_xr v_yl v_yr), 8 u_MAC, 9 v_MAC,
// 10 advect_x, 11 advect_y, 12 coeff, 13 source, 14 rho_old, 15-18 rho_xl rho_xr rho_yl rho_yr,
// 19 rho_xint, 20 rho_yint, 21-24 u_xint v_xint u_yint v_yint; host: (qx, qy)
int pyrohip_lm_stage_dump(pyrohip_state *s, int which, double *host)
{
    LM_CHECK_STATE(s);
    PYRO_REQUIRE(host, "NULL argument");
    PYRO_REQUIRE(which >= 0 && which < L_NPL - T_UXL, "which out of range");
    const Geom &g = s->g;
    PYRO_TRY(plane_to_host(s, s->work + geom_lead(g) + (size_t)(T_UXL + which) * g.plane, host));
    PYRO_CHECK_HIP(hipStreamSynchronize(s->ctx->stream));
    return 0;
}

}  // extern "C"
