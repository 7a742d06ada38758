// Tracer particles on the device: Particles.update_particles and
// enforce_particle_boundaries of pyro/particles/particles.py:213-327, with the
// bilinear interpolation of :62-86, operation by operation (this unit is built
// once, never contracted: positions agree with the reference bit for bit
// whatever arithmetic the solver's own kernels run in).
//
// One advance = three launches on the context's stream:
//   k_part_advance   one thread per live particle: midpoint update, the four
//                    sides, keep flag; per-workgroup survivor count (LDS)
//   k_part_offsets   ONE workgroup: exclusive scan of those counts, new live count
//   k_part_scatter   each workgroup scans its own flags again and writes survivor
//                    number r (old order) to slot total - 1 - r of the other buffer:
//                    the reference rebuilds its dict with popitem(), the order
//                    reverses at every update whether or not anything was dropped
// No atomics on data, no workgroup waits for another: the result is deterministic.
// Inside a device-side run (evolve.hip) the same three launches follow every step
// in their run-protocol forms (k_part_*_run): dt, "did this iteration advance" and the buffer
// parity come from device memory, the error word sticks and ends the run.
// The memory of a set is allocated and released in ctx.hip (particles_alloc /
// particles_release).
#include "common.h"

namespace pyro {

constexpr int kPartWG = 256;
static_assert(PYROHIP_PARTICLES_MAX == kPartWG * kPartWG,
              "k_part_offsets scans one per-workgroup count per thread of ONE workgroup");

struct PartGrid {
    double xmin, xmax, ymin, ymax, dx, dy;
    int bc[4];
    int mode;
    int qx, qy, ilo, jlo, pitch;
    const double *u, *v, *den;     // planes of the state (den: RATIO only)
};

// NumPy's float `%` with divisor 1 (npy_divmod): fmod, moved into [0, 1); a zero result is +0.0
__device__ inline double mod_one(double a)
{
    double m = fmod(a, 1.0);
    if (m != 0.0) {
        if (m < 0.0) m += 1.0;
    } else {
        m = 0.0;
    }
    return m;
}

// particles.py:62-86 at (x, y).  false: the 2 x 2 stencil does not lie inside the array (or the
// position is NaN / infinite) -- nothing was read
__device__ inline bool part_interp(const PartGrid &G, double x, double y, double *uo, double *vo)
{
    const double x_idx = (x - G.xmin) / G.dx - 0.5;
    const double y_idx = (y - G.ymin) / G.dy - 0.5;
    // (compared as doubles first: a NaN fails both, and nothing out of range is converted)
    if (!(x_idx > -(double)G.ilo - 1.0 && x_idx < (double)(G.qx - G.ilo))) return false;
    if (!(y_idx > -(double)G.jlo - 1.0 && y_idx < (double)(G.qy - G.jlo))) return false;
    const double xf = mod_one(x_idx), yf = mod_one(y_idx);
    // int(x_idx) truncates towards zero while the fraction of -1 < x_idx < 0 is 1 + x_idx: the
    // reference's behaviour, kept
    const long long i = (long long)trunc(x_idx) + G.ilo;
    const long long j = (long long)trunc(y_idx) + G.jlo;
    if (i < 0 || i > G.qx - 2 || j < 0 || j > G.qy - 2) return false;
    const size_t k00 = (size_t)i * G.pitch + (size_t)j, k10 = k00 + G.pitch;
    double u00 = G.u[k00], u10 = G.u[k10], u01 = G.u[k00 + 1], u11 = G.u[k10 + 1];
    double v00 = G.v[k00], v10 = G.v[k10], v01 = G.v[k00 + 1], v11 = G.v[k10 + 1];
    if (G.mode == PYROHIP_PART_VEL_RATIO) {
        const double d00 = G.den[k00], d10 = G.den[k10], d01 = G.den[k00 + 1], d11 = G.den[k10 + 1];
        u00 = u00 / d00; u10 = u10 / d10; u01 = u01 / d01; u11 = u11 / d11;
        v00 = v00 / d00; v10 = v10 / d10; v01 = v01 / d01; v11 = v11 / d11;
    }
    const double w00 = (1.0 - xf) * (1.0 - yf), w10 = xf * (1.0 - yf), w01 = (1.0 - xf) * yf,
                 w11 = xf * yf;
    *uo = ((w00 * u00 + w10 * u10) + w01 * u01) + w11 * u11;
    *vo = ((w00 * v00 + w10 * v10) + w01 * v01) + w11 * v11;
    return true;
}

// one side of enforce_particle_boundaries (particles.py:259-327) on coordinate c
__device__ inline void part_side(double &c, bool &keep, bool below, int kind, double lo, double hi)
{
    if (!keep || !(below ? (c < lo) : (c > hi))) return;
    if (kind == PYROHIP_PART_DROP) keep = false;
    else if (kind == PYROHIP_PART_PERIODIC) c = below ? (hi + c) - lo : (lo + c) - hi;
    else c = below ? 2.0 * lo - c : 2.0 * hi - c;
}

// inclusive scan of one int per thread over the workgroup (Hillis-Steele in LDS)
__device__ inline int wg_scan_incl(int v, int *sh)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < kPartWG; d <<= 1) {
        const int a = (t >= d) ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    return sh[t];
}

// candidate position and velocity of the live particles of `cur` into the candidate arrays (same
// slot: cand = positions, cand + 2 cap = velocities), keep flags, the survivors of each workgroup
// (flag: the state's flag word of a device-side run, raised with the error word; else nullptr)
__device__ __forceinline__ void part_advance_wg(const double *__restrict__ cur, double *__restrict__ cand,
                                                int cap, int n, int *__restrict__ keepf,
                                                int *__restrict__ wg_count, int *__restrict__ err,
                                                int *flag, const PartGrid &G, double dt, int *sh)
{
    if ((int)(blockIdx.x * kPartWG) >= n) return;      // the whole workgroup (uniform)
    const int t = blockIdx.x * kPartWG + threadIdx.x;
    int kf = 0;
    if (t < n) {
        const double x0 = cur[2 * (size_t)t], y0 = cur[2 * (size_t)t + 1];
        double u = 0.0, v = 0.0, x = x0, y = y0;
        bool ok = part_interp(G, x0, y0, &u, &v);
        if (ok) {
            const double hdt = 0.5 * dt;
            const double xh = x0 + u * hdt, yh = y0 + v * hdt;
            ok = part_interp(G, xh, yh, &u, &v);
        }
        bool keep = true;
        if (ok) {
            x = x0 + u * dt;
            y = y0 + v * dt;
            part_side(x, keep, true, G.bc[0], G.xmin, G.xmax);
            part_side(x, keep, false, G.bc[1], G.xmin, G.xmax);
            part_side(y, keep, true, G.bc[2], G.ymin, G.ymax);
            part_side(y, keep, false, G.bc[3], G.ymin, G.ymax);
        } else {
            atomicOr(err, 1);
            if (flag) atomicOr(flag, 1);
        }
        double *np = cand, *nv = cand + 2 * (size_t)cap;
        np[2 * (size_t)t] = x; np[2 * (size_t)t + 1] = y;
        nv[2 * (size_t)t] = u; nv[2 * (size_t)t + 1] = v;
        kf = keep ? 1 : 0;
        keepf[t] = kf;
    }
    const int tot = wg_scan_incl(kf, sh);
    if (threadIdx.x == kPartWG - 1) wg_count[blockIdx.x] = tot;
}
__global__ __launch_bounds__(kPartWG) void k_part_advance(const double *__restrict__ cur,
                                                          double *__restrict__ cand, int cap,
                                                          const int *__restrict__ count,
                                                          int *__restrict__ keepf,
                                                          int *__restrict__ wg_count,
                                                          int *__restrict__ err, PartGrid G, double dt)
{
    __shared__ int sh[kPartWG];
    part_advance_wg(cur, cand, cap, *count, keepf, wg_count, err, nullptr, G, dt, sh);
}

// exclusive scan of the per-workgroup counts (at most kPartWG of them: one per thread), the new
// live count into count_new
__device__ __forceinline__ void part_offsets_wg(int n, const int *__restrict__ wg_count,
                                                int *__restrict__ wg_off, int *__restrict__ count_new, int *sh)
{
    const int nwg = (n + kPartWG - 1) / kPartWG;
    const int t = threadIdx.x;
    const int c = (t < nwg) ? wg_count[t] : 0;
    const int incl = wg_scan_incl(c, sh);
    if (t < nwg) wg_off[t] = incl - c;
    if (t == kPartWG - 1) *count_new = incl;
}
__global__ __launch_bounds__(kPartWG) void k_part_offsets(const int *__restrict__ count,
                                                          const int *__restrict__ wg_count,
                                                          int *__restrict__ wg_off,
                                                          int *__restrict__ count_new)
{
    __shared__ int sh[kPartWG];
    part_offsets_wg(*count, wg_count, wg_off, count_new, sh);
}

// survivor number r (old order) -> slot total - 1 - r of the other buffer `out`: candidate position
// and velocity, initial position from `cur`.  (The candidates have arrays of their own: a slot of
// `out` is written while another workgroup may not have read its own candidate yet.)
__device__ __forceinline__ void part_scatter_wg(const double *__restrict__ cur, const double *__restrict__ cand,
                                                double *__restrict__ out, int cap, int n, int n_new,
                                                const int *__restrict__ keepf,
                                                const int *__restrict__ wg_off, int *sh)
{
    if ((int)(blockIdx.x * kPartWG) >= n) return;
    const int t = blockIdx.x * kPartWG + threadIdx.x;
    const int kf = (t < n) ? keepf[t] : 0;
    const int incl = wg_scan_incl(kf, sh);
    if (!kf) return;
    const int r = wg_off[blockIdx.x] + incl - 1;
    const size_t d = (size_t)(n_new - 1 - r), s = (size_t)t;
    const double *ci = cur + 2 * (size_t)cap;
    const double *cp = cand, *cv = cand + 2 * (size_t)cap;
    double *op = out, *oi = out + 2 * (size_t)cap, *ov = out + 4 * (size_t)cap;
    op[2 * d] = cp[2 * s]; op[2 * d + 1] = cp[2 * s + 1];
    oi[2 * d] = ci[2 * s]; oi[2 * d + 1] = ci[2 * s + 1];
    ov[2 * d] = cv[2 * s]; ov[2 * d + 1] = cv[2 * s + 1];
}
__global__ __launch_bounds__(kPartWG) void k_part_scatter(const double *__restrict__ cur,
                                                          const double *__restrict__ cand,
                                                          double *__restrict__ out, int cap,
                                                          const int *__restrict__ count,
                                                          const int *__restrict__ count_new,
                                                          const int *__restrict__ keepf,
                                                          const int *__restrict__ wg_off)
{
    __shared__ int sh[kPartWG];
    part_scatter_wg(cur, cand, out, cap, *count, *count_new, keepf, wg_off, sh);
}

// ---- the run-protocol forms (a device-side run: evolve.hip) ----
// What the three launches behind the step of iteration m take from device memory instead of from
// the host: S->dt (the dt the step kernel used), whether the iteration advanced the state at all,
// and which of the set's two buffers is live.
struct PartRun {
    const StepScalars *S;     // of this iteration: written by the policy call in front of the step
    int *flag;                // the state's flag word (bit 1: the step kernels', an earlier particle error)
    double *buf[2];           // buf[0]: the live buffer when the run was opened
    int *count[2];            // ... and their live counts
};
// Did iteration m advance the state?  Not past tmax or on a dead run (S->active == 0: the policy
// call), not when the step kernel has just found its state invalid or an earlier advance of this
// launch a particle outside the array (bit 1 of the flag: the next policy call makes it S->dead).
// Then nothing is stored at all.  ONE thread reads the flag for the workgroup: other workgroups
// of k_part_advance_run may be raising it, and the workgroup's barriers need one answer.
__device__ __forceinline__ bool part_run_on(const PartRun &R, int *sh)
{
    if (threadIdx.x == 0) sh[0] = (R.S->active != 0 && (*(volatile int *)R.flag & 1) == 0) ? 1 : 0;
    __syncthreads();
    const bool on = sh[0] != 0;
    __syncthreads();          // (sh is the scan's next)
    return on;
}
// the live buffer: advances so far in this run = steps that advanced the state (S->steps), each
// of which exchanged the two
__device__ __forceinline__ int part_run_live(const PartRun &R) { return R.S->steps & 1; }

__global__ __launch_bounds__(kPartWG) void k_part_advance_run(PartRun R, double *__restrict__ cand, int cap,
                                                              int *__restrict__ keepf,
                                                              int *__restrict__ wg_count,
                                                              int *__restrict__ err, PartGrid G)
{
    __shared__ int sh[kPartWG];
    if (!part_run_on(R, sh)) return;
    const int b = part_run_live(R);
    part_advance_wg(R.buf[b], cand, cap, *R.count[b], keepf, wg_count, err, R.flag, G, R.S->dt, sh);
}
__global__ __launch_bounds__(kPartWG) void k_part_offsets_run(PartRun R, const int *__restrict__ wg_count,
                                                              int *__restrict__ wg_off)
{
    __shared__ int sh[kPartWG];
    if (!part_run_on(R, sh)) return;
    const int b = part_run_live(R);
    part_offsets_wg(*R.count[b], wg_count, wg_off, R.count[b ^ 1], sh);
}
__global__ __launch_bounds__(kPartWG) void k_part_scatter_run(PartRun R, const double *__restrict__ cand,
                                                              int cap, const int *__restrict__ keepf,
                                                              const int *__restrict__ wg_off)
{
    __shared__ int sh[kPartWG];
    if (!part_run_on(R, sh)) return;
    const int b = part_run_live(R);
    part_scatter_wg(R.buf[b], cand, R.buf[b ^ 1], cap, *R.count[b], *R.count[b ^ 1], keepf, wg_off, sh);
}

}  // namespace pyro

using namespace pyro;

static int part_live(const pyrohip_particles *p, const char *fn)
{
    if (!p) { set_error(std::string(fn) + ": NULL particle set"); return PYROHIP_ERR_ARG; }
    if (!p->ctx) { set_error(std::string(fn) + ": the context of this particle set was shut down"); return PYROHIP_ERR_ARG; }
    return 0;
}

#define PART_REQUIRE(cond, msg)                                               \
    do {                                                                      \
        if (!(cond)) {                                                        \
            set_error(std::string(fn) + ": " + (msg));                        \
            return PYROHIP_ERR_ARG;                                           \
        }                                                                     \
    } while (0)

namespace pyro {

int particles_check(const pyrohip_particles *p, const pyrohip_state *s, const pyrohip_particle_params *P,
                    const char *fn)
{
    PYRO_TRY(part_live(p, fn));
    PART_REQUIRE(s && P, "NULL argument");
    PART_REQUIRE(P->size == sizeof(pyrohip_particle_params),
                 "pyrohip_particle_params.size is not the size this library was built with");
    PART_REQUIRE(s->ctx == p->ctx, "state and particle set live on different contexts");
    PART_REQUIRE(P->vel_mode == PYROHIP_PART_VEL_PLANES || P->vel_mode == PYROHIP_PART_VEL_RATIO,
                 "bad velocity mode");
    const int nidx = P->vel_mode == PYROHIP_PART_VEL_RATIO ? 3 : 2;
    for (int k = 0; k < nidx; k++)
        PART_REQUIRE(P->idx[k] >= 0 && P->idx[k] < s->nvar, "plane index out of range");
    for (int k = 0; k < 4; k++)
        PART_REQUIRE(P->bc[k] >= PYROHIP_PART_DROP && P->bc[k] <= PYROHIP_PART_MIRROR,
                     "bad particle boundary kind");
    return 0;
}

// the grid and the velocity planes of the state's CURRENT buffer, as the kernels take them
static PartGrid part_grid(const pyrohip_state *s, const pyrohip_particle_params *P)
{
    const Geom &g = s->g;
    PartGrid G;
    G.xmin = P->xmin; G.xmax = P->xmax; G.ymin = P->ymin; G.ymax = P->ymax; G.dx = P->dx; G.dy = P->dy;
    for (int k = 0; k < 4; k++) G.bc[k] = P->bc[k];
    G.mode = P->vel_mode;
    G.qx = g.qx; G.qy = g.qy; G.ilo = g.ilo; G.jlo = g.jlo; G.pitch = g.pitch;
    G.u = s->d + (size_t)P->idx[0] * g.plane;
    G.v = s->d + (size_t)P->idx[1] * g.plane;
    G.den = P->vel_mode == PYROHIP_PART_VEL_RATIO ? s->d + (size_t)P->idx[2] * g.plane : nullptr;
    return G;
}

int particles_run_advance(pyrohip_particles *p, pyrohip_state *s, const pyrohip_particle_params *P,
                          const StepScalars *S, int live0)
{
    pyrohip_ctx *c = p->ctx;
    const PartGrid G = part_grid(s, P);
    PartRun R;
    R.S = S;
    R.flag = s->d_flag;
    for (int k = 0; k < 2; k++) { R.buf[k] = p->buf[live0 ^ k]; R.count[k] = p->count + (live0 ^ k); }
    PYRO_LAUNCH(c, "k_part_advance_run", k_part_advance_run, dim3(p->nwg), dim3(kPartWG), 0, R, p->cand, p->cap,
                p->keep, p->wg_count, p->err, G);
    PYRO_LAUNCH(c, "k_part_offsets_run", k_part_offsets_run, dim3(1), dim3(kPartWG), 0, R,
                (const int *)p->wg_count, p->wg_off);
    PYRO_LAUNCH(c, "k_part_scatter_run", k_part_scatter_run, dim3(p->nwg), dim3(kPartWG), 0, R,
                (const double *)p->cand, p->cap, (const int *)p->keep, (const int *)p->wg_off);
    PYRO_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace pyro

extern "C" {

int pyrohip_particles_create(pyrohip_ctx *c, int n, const double *pos, const double *init,
                             pyrohip_particles **out)
{
    PYRO_REQUIRE(c && out && pos, "NULL argument");
    PYRO_REQUIRE(n >= 1, "a particle set holds at least one particle");
    PYRO_REQUIRE(n <= PYROHIP_PARTICLES_MAX,
                 "more than PYROHIP_PARTICLES_MAX (65536) particles: the survivor counts of the "
                 "workgroups are scanned by one workgroup");
    PYRO_CHECK_HIP(hipSetDevice(c->device));
    pyrohip_particles *p = nullptr;
    PYRO_TRY(particles_alloc(c, n, &p));
    const int rc = pyrohip_particles_upload(p, n, pos, init, nullptr);
    if (rc != 0) { (void)particles_release(p); return rc; }
    *out = p;
    return 0;
}

int pyrohip_particles_destroy(pyrohip_particles *p)
{
    if (!p) return 0;
    return particles_release(p);
}

int pyrohip_particles_upload(pyrohip_particles *p, int n, const double *pos, const double *init,
                             const double *vel)
{
    PYRO_TRY(part_live(p, __func__));
    PYRO_REQUIRE(n >= 0 && n <= p->cap, "particle count beyond the capacity of the set");
    PYRO_REQUIRE(pos || n == 0, "NULL positions");
    pyrohip_ctx *c = p->ctx;
    PYRO_CHECK_HIP(hipSetDevice(c->device));
    double *b = p->buf[p->cur];
    const size_t bytes = (size_t)2 * n * sizeof(double), cap2 = (size_t)2 * p->cap;
    if (n > 0) {
        PYRO_CHECK_HIP(hipMemcpyAsync(b, pos, bytes, hipMemcpyHostToDevice, c->stream));
        PYRO_CHECK_HIP(hipMemcpyAsync(b + cap2, init ? init : pos, bytes, hipMemcpyHostToDevice, c->stream));
        if (vel) PYRO_CHECK_HIP(hipMemcpyAsync(b + 2 * cap2, vel, bytes, hipMemcpyHostToDevice, c->stream));
        else PYRO_CHECK_HIP(hipMemsetAsync(b + 2 * cap2, 0, bytes, c->stream));
    }
    PYRO_CHECK_HIP(hipMemcpyAsync(p->count + p->cur, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
    PYRO_CHECK_HIP(hipStreamSynchronize(c->stream));      // the host arrays (and n) are borrowed
    return 0;
}

int pyrohip_particles_count(pyrohip_particles *p, int *n)
{
    PYRO_TRY(part_live(p, __func__));
    PYRO_REQUIRE(n, "NULL argument");
    pyrohip_ctx *c = p->ctx;
    PYRO_CHECK_HIP(hipSetDevice(c->device));
    PYRO_CHECK_HIP(hipMemcpyAsync(c->reduce_host, p->count + p->cur, sizeof(int), hipMemcpyDeviceToHost,
                                  c->stream));
    PYRO_CHECK_HIP(hipStreamSynchronize(c->stream));
    *n = *(int *)c->reduce_host;
    return 0;
}

int pyrohip_particles_download(pyrohip_particles *p, int *n, double *pos, double *init, double *vel)
{
    int live = 0;
    PYRO_TRY(pyrohip_particles_count(p, &live));
    PYRO_REQUIRE(live >= 0 && live <= p->cap, "corrupt live count");
    pyrohip_ctx *c = p->ctx;
    const double *b = p->buf[p->cur];
    const size_t bytes = (size_t)2 * live * sizeof(double), cap2 = (size_t)2 * p->cap;
    double *dst[3] = {pos, init, vel};
    for (int k = 0; k < 3; k++)
        if (dst[k] && live > 0)
            PYRO_CHECK_HIP(hipMemcpyAsync(dst[k], b + k * cap2, bytes, hipMemcpyDeviceToHost, c->stream));
    PYRO_CHECK_HIP(hipStreamSynchronize(c->stream));
    if (n) *n = live;
    return 0;
}

int pyrohip_particles_advance(pyrohip_particles *p, pyrohip_state *s,
                              const pyrohip_particle_params *P, double dt)
{
    PYRO_TRY(particles_check(p, s, P, __func__));
    pyrohip_ctx *c = p->ctx;
    PYRO_CHECK_HIP(hipSetDevice(c->device));
    PYRO_TRY(comm_wait_halo(s));
    const PartGrid G = part_grid(s, P);
    const double *cur = p->buf[p->cur];
    double *nxt = p->buf[p->cur ^ 1];
    const int *cnt = p->count + p->cur;
    int *cnt_new = p->count + (p->cur ^ 1);
    PYRO_CHECK_HIP(hipMemsetAsync(p->err, 0, sizeof(int), c->stream));
    PYRO_LAUNCH(c, "k_part_advance", k_part_advance, dim3(p->nwg), dim3(kPartWG), 0, cur, p->cand, p->cap, cnt,
                p->keep, p->wg_count, p->err, G, dt);
    PYRO_LAUNCH(c, "k_part_offsets", k_part_offsets, dim3(1), dim3(kPartWG), 0, cnt,
                (const int *)p->wg_count, p->wg_off, cnt_new);
    PYRO_LAUNCH(c, "k_part_scatter", k_part_scatter, dim3(p->nwg), dim3(kPartWG), 0, cur,
                (const double *)p->cand, nxt, p->cap, cnt, (const int *)cnt_new, (const int *)p->keep,
                (const int *)p->wg_off);
    PYRO_CHECK_HIP(hipGetLastError());
    // what comes back: the error word (no particle or state data crosses to the host)
    PYRO_CHECK_HIP(hipMemcpyAsync(c->reduce_host, p->err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PYRO_CHECK_HIP(hipStreamSynchronize(c->stream));
    if (*(int *)c->reduce_host != 0) {
        // (the live buffer was only read: the set is the one before the call)
        set_error("a particle's interpolation stencil leaves the state's array (position outside "
                  "the ghosted grid, NaN or infinite): the particle set is unchanged");
        return PYROHIP_ERR_STATE;
    }
    p->cur ^= 1;
    return 0;
}

}  // extern "C"
