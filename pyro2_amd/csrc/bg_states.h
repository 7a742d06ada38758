// The per-cell arithmetic of the unsplit CTU predictor for (u, v) of burgers_interface.py:4-312,
// shared by the staged kernels (incompressible.hip: burgers with gpu.kernel_set = 0, burgers_viscous
// and the incompressible solvers) and the one-launch burgers step (burgers.hip).  Every expression
// keeps the reference's operation order; compiled with -ffp-contract=off both users get the same bits.
#pragma once
#include "stencil.h"

namespace pyro {

// burgers_interface.py:265-290
__device__ __forceinline__ double bg_riemann(double ql, double qr)
{
    if (ql <= 0.0 && qr >= 0.0) return 0.0;
    return (ql > 0.0 && ql + qr > 0.0) ? ql : qr;
}
// burgers_interface.py:236-262
__device__ __forceinline__ double bg_upwind(double ql, double qr, double s)
{
    if (s == 0.0) return 0.5 * (ql + qr);
    return (s > 0.0) ? ql : qr;
}

// get_interface_states (burgers_interface.py:4-86): the uncorrected ("hat") states one cell sends
// to its faces for a component q with limited slopes ldx / ldy, advected by the cell's (uc, vc):
// xl sits on the cell's HIGH x face (the left state there), xr on its low x face, yl / yr likewise
struct BgHat { double xl, xr, yl, yr; };
__device__ __forceinline__ BgHat bg_hat(double q, double ldx, double ldy, double uc, double vc,
                                        double dtdx, double dtdy)
{
    BgHat h;
    h.xl = q + 0.5 * (1.0 - dtdx * uc) * ldx;
    h.xr = q - 0.5 * (1.0 + dtdx * uc) * ldx;
    h.yl = q + 0.5 * (1.0 - dtdy * vc) * ldy;
    h.yr = q - 0.5 * (1.0 + dtdy * vc) * ldy;
    return h;
}

// apply_transverse_corrections (burgers_interface.py:89-175) over one cell: the advecting
// component's hat states on the cell's low (0) and high (1) transverse face (ql / qr) and those of
// the two carried components a, b -> the terms added to both states of a and of b
__device__ __forceinline__ void bg_transverse(double dtd, double ql0, double qr0, double ql1, double qr1,
                                              double al0, double ar0, double al1, double ar1,
                                              double bl0, double br0, double bl1, double br1,
                                              double &ta, double &tb)
{
    const double h0 = bg_riemann(ql0, qr0), h1 = bg_riemann(ql1, qr1);
    const double bar = 0.5 * (h0 + h1);
    const double a0 = bg_upwind(al0, ar0, h0), a1 = bg_upwind(al1, ar1, h1);
    const double b0 = bg_upwind(bl0, br0, h0), b1 = bg_upwind(bl1, br1, h1);
    ta = -0.5 * dtd * bar * (a1 - a0);
    tb = -0.5 * dtd * bar * (b1 - b0);
}

// riemann_and_upwind (burgers_interface.py:293-312): the MAC velocity of a face from the corrected
// states of the normal component
__device__ __forceinline__ double bg_mac(double l, double r) { return bg_upwind(l, r, bg_riemann(l, r)); }
// construct_unsplit_fluxes (burgers_interface.py:178-233): the flux of a component through that face
__device__ __forceinline__ double bg_flux(double l, double r, double mac) { return 0.5 * bg_upwind(l, r, mac) * mac; }

}  // namespace pyro
