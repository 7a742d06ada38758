// The limiter of McCorquodale & Colella for one cell, shared by the fourth-order units
// (comp_fv4.hip: the primitive variables of compressible_fv4 / compressible_sdc;
// advection_rk.hip: the scalar of advection_fv4).  The reference's operation order, so that a
// unit compiled with -ffp-contract=off gives numba's bits.
#pragma once
#include <hip/hip_runtime.h>

namespace pyro {

// mesh/fourth_order.py:97-131 (x) / :186-220 (y): the limiter of the cell c with the window
// w[0..6] = a[c-3 .. c+3]; returns ar[c] (its lower face) and al[c+1] (its upper face).
// d3a_top_zero: d3a[c+2] is one the reference never fills (the y sweep's last cell, :176-179).
__device__ __forceinline__ void mc_limit(const double *w, bool d3a_top_zero, double &ar_c,
                                         double &al_c1)
{
    const double C2 = 1.25, C3 = 0.1;
    const double aint_c = (7.0 / 12.0) * (w[2] + w[3]) - (1.0 / 12.0) * (w[1] + w[4]);
    const double aint_c1 = (7.0 / 12.0) * (w[3] + w[4]) - (1.0 / 12.0) * (w[2] + w[5]);
    ar_c = aint_c;
    al_c1 = aint_c1;
    const double a = w[3];
    const double dafm = a - aint_c, dafp = aint_c1 - a;
    const double d2af = 6.0 * (aint_c - 2.0 * a + aint_c1);
    double d2ac[5];   // cells c-2 .. c+2
#pragma unroll
    for (int k = 0; k < 5; k++) d2ac[k] = w[k] - 2.0 * w[k + 1] + w[k + 2];
    if (dafm * dafp <= 0.0 || (a - w[1]) * (w[5] - a) <= 0.0) {
        const double s = copysign(1.0, d2ac[2]);
        double d2a_lim;
        if (s == copysign(1.0, d2ac[1]) && s == copysign(1.0, d2ac[3]) && s == copysign(1.0, d2af))
            d2a_lim = s * fmin(fmin(fmin(fabs(d2af), C2 * fabs(d2ac[1])), C2 * fabs(d2ac[2])),
                               C2 * fabs(d2ac[3]));
        else
            d2a_lim = 0.0;
        const double amax = fmax(fmax(fmax(fmax(fabs(w[1]), fabs(w[2])), fabs(w[3])), fabs(w[4])),
                                 fabs(w[5]));
        const double rho = (fabs(d2af) <= 1.e-12 * amax) ? 0.0 : d2a_lim / d2af;
        if (rho < 1.0 - 1.e-12) {
            // d3a at cells c-1 .. c+2
            const double d0 = d2ac[1] - d2ac[0], d1 = d2ac[2] - d2ac[1], d2 = d2ac[3] - d2ac[2];
            const double d3 = d3a_top_zero ? 0.0 : d2ac[4] - d2ac[3];
            const double d3a_min = fmin(fmin(fmin(d0, d1), d2), d3);
            const double d3a_max = fmax(fmax(fmax(d0, d1), d2), d3);
            if (C3 * fmax(fabs(d3a_min), fabs(d3a_max)) <= (d3a_max - d3a_min)) {
                if (dafm * dafp < 0.0) {
                    ar_c = a - rho * dafm;
                    al_c1 = a + rho * dafp;
                } else if (fabs(dafm) >= 2.0 * fabs(dafp)) {
                    ar_c = a - 2.0 * (1.0 - rho) * dafp - rho * dafm;
                } else if (fabs(dafp) >= 2.0 * fabs(dafm)) {
                    al_c1 = a + 2.0 * (1.0 - rho) * dafm + rho * dafp;
                }
            }
        }
    } else {
        if (fabs(dafm) >= 2.0 * fabs(dafp)) ar_c = a - 2.0 * dafp;
        if (fabs(dafp) >= 2.0 * fabs(dafm)) al_c1 = a + 2.0 * dafm;
    }
}

}  // namespace pyro
