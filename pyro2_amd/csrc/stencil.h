// Per-cell stencil arithmetic shared by the advection and compressible
// kernels.  Every expression keeps the reference's operation order so that,
// compiled with -ffp-contract=off, results are bit-identical to NumPy/numba
// (SURVEY.md 8(a) "arithmetic-order rules").
#pragma once
#include <hip/hip_runtime.h>

#include "builds.h"

namespace pyro {

// MC limiter building block, pyro/mesh/reconstruction.py:84-91 / 113-120
__device__ __forceinline__ double mc_select(double dc, double dl, double dr)
{
    double d1 = 2.0 * ((fabs(dl) < fabs(dr)) ? dl : dr);
    double dt = (fabs(dc) < fabs(d1)) ? dc : d1;
    return (dl * dr > 0.0) ? dt : 0.0;
}

// limit2 (reconstruction.py:69-91) at the centre of (am, a0, ap)
__device__ __forceinline__ double limit2(double am, double a0, double ap)
{
    double dc = 0.5 * (ap - am);
    double dl = ap - a0;
    double dr = a0 - am;
    // where dl*dr > 0 the three candidates share their sign (dc is their
    // mean), so the selects by magnitude of mc_select are two minima of
    // absolute values (v_min_f64 with |.| operand modifiers) and a sign copy:
    // the SAME candidate is chosen, bit for bit (ties have equal values), at 8
    // instead of 11 VALU instructions (3 compares + 6 v_cndmask_b32 there)
    const double m = fmin(fabs(dl), fabs(dr));
    const double r = copysign(fmin(fabs(dc), m + m), dl);
    return (dl * dr > 0.0) ? r : 0.0;
}

// mc_select(dc, dl, dr) for the FOURTH-ORDER centred slope of limit4,
// dc = (2/3) (ap1 - am1 - 0.25 (l2p + l2m)) with l2p / l2m the limit2 slopes of the two
// neighbours, as two minima of magnitudes and a sign copy (like limit2 above).  Where
// dl * dr > 0 this dc shares the sign of dl and dr: |l2p| <= 2 |dl| and |l2m| <= 2 |dr|
// (as computed: m + m of the rounded differences), so 0.25 (l2p + l2m) stays below
// 0.5 (1 + eps) (|dl| + |dr|) and can neither turn the sign of ap1 - am1 nor cancel it.
// The SAME candidate comes out, bit for bit, at 8 instead of 11 vector instructions
// (3 compares + 6 v_cndmask_b32 in mc_select).
__device__ __forceinline__ double mc_select_l4(double dc, double dl, double dr)
{
    const double m = fmin(fabs(dl), fabs(dr));
    const double r = copysign(fmin(fabs(dc), m + m), dl);
    return (dl * dr > 0.0) ? r : 0.0;
}

// limited slope at the centre of the 5-point stencil (reconstruction.py:9-120)
//   limiter 0: nolimit, 1: limit2, otherwise limit4
__device__ __forceinline__ double limited_slope(double am2, double am1, double a0, double ap1,
                                                double ap2, int limiter)
{
    if (limiter == 0) return 0.5 * (ap1 - am1);
    if (limiter == 1) return limit2(am1, a0, ap1);
    double l2p = limit2(a0, ap1, ap2);
    double l2m = limit2(am2, am1, a0);
    double dc = (2. / 3.) * (ap1 - am1 - 0.25 * (l2p + l2m));
    double dl = ap1 - a0;
    double dr = a0 - am1;
    return mc_select_l4(dc, dl, dr);
}

// limit4 at the centre of (am1, a0, ap1) from the limit2 slopes of the two neighbours -- the
// expression above with l2m = limit2(am2, am1, a0), l2p = limit2(a0, ap1, ap2) handed in: a
// marching kernel computes every cell's centred limit2 ONCE and takes the neighbours' from the
// row window / the neighbouring lanes (same function, same operands: the same bits)
__device__ __forceinline__ double limit4_from(double l2m, double l2p, double am1, double a0, double ap1)
{
    const double dc = (2. / 3.) * (ap1 - am1 - 0.25 * (l2p + l2m));
    return mc_select_l4(dc, ap1 - a0, a0 - am1);
}

// Contracted builds of the row-marching kernels (round 6): the MC-limited slopes as HALF slopes in signed
// min / max form -- no sign copy, no product of the one-sided differences, no compare + selects.
// With lo = min(dl, dr), hi = max(dl, dr), a = max(lo, 0), b = min(hi, 0):
//     limit2 / 2 = max(min((ap - am) / 4, a), b)
// (both differences positive: b = 0 and min(dc / 2, lo) > 0; both negative: a = 0, min(dc / 2, 0) =
// dc / 2 and max(dc / 2, hi); of opposite signs or one of them zero: a = b = 0 and the result is 0),
// and the same with the fourth-order centred slope of limit4 in place of (ap - am) / 4 -- mc_select_l4
// above shows that where dl dr > 0 it shares their sign.  Scaling by the power of two is
// exact: 2 x the result equals limit2 / limit4 up to the rounding of the centred
// difference's factors ((2/3) x vs 2 (1/3) x).  12 + 7 -> 10 + 5 instructions per variable and direction.
__device__ __forceinline__ void half_clip(double dl, double dr, double &a, double &b)
{
    a = fmax(fmin(dl, dr), 0.0);
    b = fmin(fmax(dl, dr), 0.0);
}
__device__ __forceinline__ double half_limit2(double am, double a0, double ap)
{
    double a, b;
    half_clip(ap - a0, a0 - am, a, b);
    return fmax(fmin(0.25 * (ap - am), a), b);
}
// half of limit4_from(): h2m / h2p = half_limit2 of the lower neighbour, the upper one
__device__ __forceinline__ double half_limit4_from(double h2m, double h2p, double am1, double a0, double ap1)
{
    double a, b;
    half_clip(ap1 - a0, a0 - am1, a, b);
    return fmax(fmin((1. / 3.) * (ap1 - am1 - 0.5 * (h2p + h2m)), a), b);
}

// blockIdx -> logical tile id such that each XCD (blocks are dealt round-robin
// to the 8 XCDs, MI355X_MICROARCH.md "block b runs on XCD b % 8") works on a
// contiguous band of tiles and halo re-reads hit its own L2.  Performance
// only: any mapping is correct.
__device__ __forceinline__ int xcd_tile(int b, int nb)
{
    const int nxcd = 8;
    if (nb % nxcd != 0) return b;
    return (b % nxcd) * (nb / nxcd) + b / nxcd;
}

// 2-d version for row-per-block kernels launched as a 1-d grid of
// 8*ceil(gx*gy/8) blocks: returns false for the padding blocks, otherwise the
// logical (bx, by) with by = row index.  XCD k then owns a contiguous band of
// rows, walked in order, so the +-1..4 neighbour rows of a stencil are L2 hits
// instead of being re-fetched by every XCD (measured 4-7x FETCH_SIZE
// amplification without it, profiles/r01_*).
__device__ __forceinline__ bool xcd_block_2d(int gx, int gy, int &bx, int &by)
{
    const int N = gx * gy;
    const int per = (N + 7) / 8;
    const int L = blockIdx.x;
    const int Lp = (L % 8) * per + L / 8;
    if (Lp >= N) return false;
    bx = Lp % gx;
    by = Lp / gx;
    return true;
}
inline int xcd_grid_1d(int gx, int gy) { return 8 * ((gx * gy + 7) / 8); }

// Ghost fill as an index map (array_indexer.py:163-274 / k_fill_x, k_fill_y of
// ctx.hip): the source of array index i is a * i + b with (a, b) per side --
// outflow (0, edge), reflect (-1, mirror), periodic (1, shift); interior and
// other boundary types map to themselves.  Branch-free, so that the row map in
// the marching loop stays on the scalar unit.
// a value that is the same in every lane of the wavefront, moved to a scalar register
#if !defined(PYRO_EMU)
__device__ __forceinline__ int pyro_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
#else
__device__ __forceinline__ int pyro_uniform(int v) { return v; }
#endif

struct BcMap { int alo, blo, ahi, bhi; bool odd_lo, odd_hi; };
__host__ __device__ inline BcMap bc_map(int lo, int hi, int ng, int bl, int br, bool fill)
{
    BcMap m{1, 0, 1, 0, false, false};
    if (!fill) return m;
    if (bl == PYROHIP_BC_OUTFLOW) { m.alo = 0; m.blo = lo; }
    else if (bl == PYROHIP_BC_REFLECT_EVEN || bl == PYROHIP_BC_REFLECT_ODD) { m.alo = -1; m.blo = 2 * ng - 1; }
    else if (bl == PYROHIP_BC_PERIODIC) { m.alo = 1; m.blo = hi - ng + 1; }
    if (br == PYROHIP_BC_OUTFLOW) { m.ahi = 0; m.bhi = hi; }
    else if (br == PYROHIP_BC_REFLECT_EVEN || br == PYROHIP_BC_REFLECT_ODD) { m.ahi = -1; m.bhi = 2 * hi + 1; }
    else if (br == PYROHIP_BC_PERIODIC) { m.ahi = 1; m.bhi = ng - hi - 1; }
    m.odd_lo = (bl == PYROHIP_BC_REFLECT_ODD);
    m.odd_hi = (br == PYROHIP_BC_REFLECT_ODD);
    return m;
}
__device__ __forceinline__ int bc_src(const BcMap &m, int i, int lo, int hi)
{
    return i < lo ? m.alo * i + m.blo : (i > hi ? m.ahi * i + m.bhi : i);
}

// hse boundary of the compressible solver, energy (compressible/BC.py:64-84 lower y side, :95-115
// upper): the pressure of the last interior cell integrated outwards at constant density
// (dp = rho g dy), its kinetic energy kept.  hse_start: that cell; hse_next: the energy of the next
// ghost cell away from it.  IEEE operations in the reference's order, never contracted (fp_keep):
// the variable-by-variable fill (k_fill_y_user, ctx.hip) and the one-launch frame fill of a
// device-side run (k_fill_frame2_user, compressible.hip, both arithmetic builds) give the same bits.
// fp_keep: a product that must stay a product.  A unit compiled with -ffp-contract=fast fuses it
// into the sum it feeds whatever pragma surrounds it; the value passes through an empty asm
// statement, which the instruction selector does not look through.
__device__ __forceinline__ double fp_keep(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(x));
#endif
    return x;
}
struct HseMarch { double pres, dens, ke; };
__device__ __forceinline__ HseMarch hse_start(double dens, double ener, double xm, double ym, double gamma)
{
    HseMarch h;
    h.dens = dens;
    h.ke = 0.5 * (fp_keep(xm * xm) + fp_keep(ym * ym)) / dens;
    const double eint = (ener - h.ke) / dens;
    h.pres = dens * eint * (gamma - 1.0);                          // eos.pres
    return h;
}
__device__ __forceinline__ double hse_next(HseMarch &h, bool upper, double gamma, double grav, double dy)
{
    const double dp = fp_keep(grav * h.dens * dy);
    h.pres = upper ? h.pres + dp : h.pres - dp;
    return h.pres / (gamma - 1.0) + h.ke;                          // eos.rhoe
}

// Tile kernels that load THROUGH the ghost fill (advection_nonuniform.hip, advection_rk.hip):
// array cell (i, j) of a variable with the row / column maps mr / mc -> the offset of its interior
// source cell in the plane.  Cells beyond the array feed discarded faces only: any address inside.
// (G: the plane's geometry, common.h's Geom)
template <class G>
__device__ __forceinline__ size_t tile_src_off(const G &g, const BcMap &mr, const BcMap &mc, int i, int j)
{
    i = i < 0 ? 0 : (i > g.qx - 1 ? g.qx - 1 : i);
    j = j < 0 ? 0 : (j > g.qy - 1 ? g.qy - 1 : j);
    return (size_t)bc_src(mr, i, g.ilo, g.ihi) * g.pitch + bc_src(mc, j, g.jlo, g.jhi);
}
// ... and whether the value changes sign on the way (x fill, then y fill: the corner is the
// composition of the two odd reflections)
struct TileSrc { size_t off; bool neg; };
template <class G>
__device__ __forceinline__ TileSrc tile_src(const G &g, const BcMap &mr, const BcMap &mc, int i, int j)
{
    const size_t off = tile_src_off(g, mr, mc, i, j);
    i = i < 0 ? 0 : (i > g.qx - 1 ? g.qx - 1 : i);       // (the clamped cell lies on the same side)
    j = j < 0 ? 0 : (j > g.qy - 1 ? g.qy - 1 : j);
    const bool nr = (i < g.ilo && mr.odd_lo) || (i > g.ihi && mr.odd_hi);
    const bool nc = (j < g.jlo && mc.odd_lo) || (j > g.jhi && mc.odd_hi);
    return TileSrc{off, nr != nc};
}

}  // namespace pyro
