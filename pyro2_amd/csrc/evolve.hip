// The device-side run protocol: the small kernels between two steps of a run
// that advances without a host round trip per step -- ghost frames of both state buffers, the
// driver's dt policy -- and the three host steps every such loop is made of: evolve_open,
// evolve_between, evolve_close (common.h).  The solvers' loops (pyrohip_comp_evolve,
// pyrohip_comp_rk_evolve: comp_api.hip; pyrohip_swe_evolve: swe.hip) keep what is theirs: which
// step kernel runs, the first CFL minimum, the halo exchange.  A tracer particle set may ride along
// (DESIGN.md 15.1): evolve_bind_particles before the open, evolve_particles behind every step.
#include "common.h"
#include "stencil.h"

using namespace pyro;

// Boundary fill of all NV variables (4: the hydro states; 2: burgers' u, v) AND the ghost frame of the other state buffer in one
// launch (device-side stepping with the row-marching kernel: pyrohip_fill_bc is two launches,
// the copy of the ghost frame into the new buffer a third -- 19 us of kernels and two gaps per
// step, 2.5 % of a 4096^2 step, 8 % at 2048^2).  A ghost cell's value goes through the x rule
// and then the y rule (array_indexer.py:163-274 fills x over all columns first, so a corner
// takes its value from an x ghost cell): for outflow / reflect / periodic sides both are index
// maps with a sign, and their composition is what the two passes leave.  One thread per
// cell of the frame.
// (b: piece of 256 threads, t: thread in the piece -- a workgroup of k_fill_frame2, or a quarter
// of one of k_fill_frame2_policy)
template <int NV>
__device__ __forceinline__ void fill_frame2_piece(const double *src, double *cur, double *alt,
                                                  const Geom &g, const int *__restrict__ bc, int b, int t)
{   // src: the buffer whose interior the images are taken from (cur itself, or -- at the end of a
    // run of one-launch steps -- the buffer that holds the previous state); alt may be nullptr
    // 1-d grid (frame_pieces, common.h): first the 2 ng full ghost rows in pieces of 256 columns,
    // then the ghost columns of the interior rows, 256 / (2 ng) rows per piece
    const int ng = g.ng;
    const int nxb = (g.qy + 255) / 256, nrowblk = 2 * ng * nxb;
    int i, j;
    if (b < nrowblk) {                              // a piece of a full ghost row
        const int rr = b / nxb;
        i = (rr < ng) ? rr : g.ihi + 1 + (rr - ng);
        j = (b - rr * nxb) * 256 + t;
        if (j >= g.qy) return;
    } else {                                        // ghost columns of interior rows
        const int rows_per_block = 256 / (2 * ng);
        const int r = (b - nrowblk) * rows_per_block + t / (2 * ng);
        const int kx = t % (2 * ng);
        if (r >= g.nx || t >= rows_per_block * 2 * ng) return;
        i = g.ilo + r;
        j = (kx < ng) ? kx : g.jhi + 1 + (kx - ng);
    }
    const size_t k = (size_t)i * g.pitch + j;
#pragma unroll
    for (int n = 0; n < NV; n++) {
        const pyro::BcMap mx = pyro::bc_map(g.ilo, g.ihi, ng, bc[n * 4 + 0], bc[n * 4 + 1], true);
        const pyro::BcMap my = pyro::bc_map(g.jlo, g.jhi, ng, bc[n * 4 + 2], bc[n * 4 + 3], true);
        const int si = pyro::bc_src(mx, i, g.ilo, g.ihi), sj = pyro::bc_src(my, j, g.jlo, g.jhi);
        const bool neg = ((i < g.ilo && mx.odd_lo) || (i > g.ihi && mx.odd_hi)) !=
                         ((j < g.jlo && my.odd_lo) || (j > g.jhi && my.odd_hi));
        const double v = src[n * g.plane + (size_t)si * g.pitch + sj];
        const double w = neg ? -v : v;
        cur[n * g.plane + k] = w;
        if (alt) alt[n * g.plane + k] = w;
    }
}
template <int NV>
__global__ __launch_bounds__(256) void k_fill_frame2(const double *src, double *cur, double *alt,
                                                     Geom g, const int *__restrict__ bc)
{
    fill_frame2_piece<NV>(src, cur, alt, g, bc, (int)blockIdx.x, (int)threadIdx.x);
}

// ghost frame of all 4 planes old -> new (the reference updates in place, so
// ghost cells keep their pre-step values)
__global__ void k_copy_frame4(const double *__restrict__ src, double *__restrict__ dst, Geom g)
{
    // 1-d grid (frame_pieces): the 2 ng full ghost rows in pieces of 256 columns, then the ghost columns of
    // the interior rows (a 2-d grid whose column part ran in block column 0 only launched
    // 33 thousand workgroups at 16384^2 for 1024 that had work)
    const int ng = g.ng;
    const int nxb = (g.qy + 255) / 256, nrowblk = 2 * ng * nxb;
    const int b = blockIdx.x;
    int i, j;
    if (b < nrowblk) {                              // a piece of a full ghost row
        const int rr = b / nxb;
        i = (rr < ng) ? rr : g.ihi + 1 + (rr - ng);
        j = (b - rr * nxb) * 256 + (int)threadIdx.x;
        if (j >= g.qy) return;
    } else {                                        // ghost columns of interior rows
        const int t = threadIdx.x;                  // 256 threads: 2*ng columns x rows
        const int rows_per_block = 256 / (2 * ng);
        const int r = (b - nrowblk) * rows_per_block + t / (2 * ng);
        const int kx = t % (2 * ng);
        if (r >= g.nx || t >= rows_per_block * 2 * ng) return;
        i = g.ilo + r;
        j = (kx < ng) ? kx : g.jhi + 1 + (kx - ng);
    }
    const size_t k = (size_t)i * g.pitch + j;
#pragma unroll
    for (int n = 0; n < 4; n++) dst[n * g.plane + k] = src[n * g.plane + k];
}
void pyro::state_copy_frame4(pyrohip_state *s)
{
    const Geom &g = s->g;
    hipLaunchKernelGGL(k_copy_frame4, dim3(frame_pieces(g)), dim3(256), 0, s->ctx->stream,
                       (const double *)s->d, s->alt_base + geom_lead(g), g);
}

constexpr int kPolicyThreads = 1024;
// The driver's compute_timestep (simulation_null.py:222-244) between two steps of a run that
// advances on the device (dt_policy_apply, common.h), from the CFL minimum the previous step
// kernel left in device memory.
__device__ __forceinline__ void dt_policy_block(StepScalars *S, const double *cflmin,
                                                const int *flag, double *dts, int slot,
                                                int final_call, const double *part, int nparts,
                                                double *minout, int flag_mask, const double *fpart,
                                                int nfpart)
{
    // the CFL minimum of the previous step: already reduced (cflmin), or still the
    // per-workgroup partials of the tile kernel (part: reduced here, kept in minout)
    // (fpart: a stratified run -- the partials of the frame cells the fill in front of this call
    // wrote; the minimum of both is the reference's, over the whole array with ghost cells filled)
    // (1024 threads, four loads in flight each: 40 000 partials at 16384^2 -- with 256 threads
    // and one dependent load after the other this took 36 us at 8192^2, 1.4 % of the step)
    __shared__ double red[kPolicyThreads];
    __shared__ double cmin_s;
    if (part != nullptr || fpart != nullptr) {
        double m0 = INFINITY, m1 = INFINITY, m2 = INFINITY, m3 = INFINITY;
        const int nt = blockDim.x;
        int i = threadIdx.x;
        for (; i + 3 * nt < nparts; i += 4 * nt) {
            const double a = part[i], b = part[i + nt], c2 = part[i + 2 * nt], d = part[i + 3 * nt];
            m0 = fmin(m0, a); m1 = fmin(m1, b); m2 = fmin(m2, c2); m3 = fmin(m3, d);
        }
        for (; i < nparts; i += nt) m0 = fmin(m0, part[i]);
        for (i = threadIdx.x; i < nfpart; i += nt) m1 = fmin(m1, fpart[i]);
        if (part == nullptr && threadIdx.x == 0) m2 = fmin(m2, *cflmin);
        const double m = fmin(fmin(m0, m1), fmin(m2, m3));
        red[threadIdx.x] = m;
        __syncthreads();
        for (int w = blockDim.x / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + w]);
            __syncthreads();
        }
        if (threadIdx.x == 0) { cmin_s = red[0]; *minout = red[0]; }
    } else if (threadIdx.x == 0) {
        cmin_s = *cflmin;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    // (raised by the step that just ran: it does not count)
    pyro::dt_policy_apply(S, cmin_s, (*flag & flag_mask) != 0, dts, slot, final_call);
}
__global__ __launch_bounds__(kPolicyThreads) void k_dt_policy(StepScalars *S, const double *cflmin,
                                                   const int *flag, double *dts, int slot,
                                                   int final_call, const double *part, int nparts,
                                                   double *minout, int flag_mask, const double *fpart,
                                                   int nfpart)
{
    dt_policy_block(S, cflmin, flag, dts, slot, final_call, part, nparts, minout, flag_mask, fpart, nfpart);
}
// The two small launches between two steps of a device-side run in ONE (round 6): the ghost
// frames of both buffers (k_fill_frame2: reads the state the last step left) and the driver's dt
// policy (k_dt_policy: reads that step's CFL partials) do not depend on each other.  Workgroups
// of 1024 threads: the first nfill hold four 256-thread pieces of the fill each, the last one
// runs the policy.  One launch and its gap less per step (8 us of a 0.68 ms step at 4096^2).
template <int NV>
__global__ __launch_bounds__(kPolicyThreads) void k_fill_frame2_policy(
    const double *src, double *cur, double *alt, Geom g, const int *__restrict__ bc, int npieces,
    StepScalars *S, const double *cflmin, const int *flag, double *dts, int slot, const double *part,
    int nparts, double *minout)
{
    if (blockIdx.x + 1 == gridDim.x) {
        dt_policy_block(S, cflmin, flag, dts, slot, 0, part, nparts, minout, 1, nullptr, 0);
        return;
    }
    const int piece = (int)blockIdx.x * 4 + (int)threadIdx.x / 256;
    if (piece < npieces) fill_frame2_piece<NV>(src, cur, alt, g, bc, piece, (int)threadIdx.x % 256);
}

// The policy between two steps of an ensemble (pyrohip_comp_evolve_batch): one
// workgroup per member does what k_dt_policy does for a single run -- the minimum of the member's CFL
// partials (kept in its minout), then dt_policy_apply on its own scalars, flag and dt slots.
__global__ __launch_bounds__(kPolicyThreads) void k_dt_policy_batch(const BatchMember *__restrict__ tab, int nparts,
                                                                    int slot, int final_call)
{
    const BatchMember M = tab[blockIdx.x];
    dt_policy_block(member_ptr(M.S), member_ptr(M.minout), member_ptr(M.flag), member_ptr(M.dts), slot, final_call,
                    member_ptr(M.part), nparts, member_ptr(M.minout), 1, nullptr, 0);
}

namespace pyro {

int evolve_batch_policy(pyrohip_ctx *c, const BatchMember *d_tab, int nmembers, int nparts, int slot, int final_call)
{
    PYRO_LAUNCH(c, "k_dt_policy_batch", k_dt_policy_batch, dim3(nmembers), dim3(kPolicyThreads), 0, d_tab, nparts,
                slot, final_call);
    PYRO_CHECK_HIP(hipGetLastError());
    return 0;
}

// the first policy call of a member: k_dt_policy on the CFL minimum of the state as handed over
int evolve_batch_policy0(pyrohip_ctx *c, const BatchMember &M, const double *dmin)
{
    PYRO_LAUNCH(c, "k_dt_policy", k_dt_policy, dim3(1), dim3(kPolicyThreads), 0, member_ptr(M.S), dmin,
                (const int *)member_ptr(M.flag), member_ptr(M.dts), 0, 0, (const double *)nullptr, 0,
                member_ptr(M.minout), 1, (const double *)nullptr, 0);
    PYRO_CHECK_HIP(hipGetLastError());
    return 0;
}

// (x sides of a slab that are cuts -- PYROHIP_BC_HALO -- are identity maps: the halo rows are data
// that arrived with the exchange, the y rule runs along them like along an interior row and the
// other buffer's frame takes a copy, which the exchange posted by the coming step overwrites)
bool frame_fill_ok(const pyrohip_state *s, bool halo_ok, bool sph_ok)
{
    if ((s->nvar != 4 && s->nvar != 2) || (s->nb_set && !halo_ok) || s->user_bc || s->ramp_bc || (s->sph && !sph_ok) || !s->alt_base)
        return false;
    for (int k = 0; k < 4 * s->nvar; k++) {
        const int b = s->bc[k];
        if (b != PYROHIP_BC_OUTFLOW && b != PYROHIP_BC_REFLECT_EVEN && b != PYROHIP_BC_REFLECT_ODD &&
            b != PYROHIP_BC_PERIODIC && !(halo_ok && (k % 4) < 2 && b == PYROHIP_BC_HALO))
            return false;
    }
    return true;
}

// k_fill_frame2: the ghost frame of the state's buffer -- and of `alt` -- from the interior at src
static int launch_frame(pyrohip_state *s, const double *src, double *alt)
{
    // (frame_fill_ok: 4 variables or 2)
    const auto kernel = s->nvar == 2 ? k_fill_frame2<2> : k_fill_frame2<4>;
    PYRO_LAUNCH(s->ctx, "k_fill_frame2", kernel, dim3(frame_pieces(s->g)), dim3(256), 0, src, s->d, alt, s->g,
                (const int *)s->d_bc);
    PYRO_CHECK_HIP(hipGetLastError());
    return 0;
}

static int launch_policy(EvolveRun &r, int slot, int final_call, int flag_mask)
{
    pyrohip_state *s = r.s;
    PYRO_LAUNCH(s->ctx, "k_dt_policy", k_dt_policy, dim3(1), dim3(kPolicyThreads), 0, r.d_scal, r.dmin,
                (const int *)s->d_flag, s->d_dts, slot, final_call, r.pend, r.pend ? r.npend : 0,
                const_cast<double *>(r.dmin), flag_mask, r.fpart, r.fpart ? r.nfpart : 0);
    PYRO_CHECK_HIP(hipGetLastError());
    r.pend = nullptr;
    r.fpart = nullptr;
    return 0;
}

int evolve_bind_particles(EvolveRun &r, pyrohip_state *s, pyrohip_particles *ps, const pyrohip_particle_params *pp,
                          const char *fn)
{
    r.ps = nullptr;
    if (!ps) return 0;
    PYRO_TRY(particles_check(ps, s, pp, fn));
    if (s->nb_set || s->sph) {
        set_error(std::string(fn) + ": tracer particles ride along on a single Cartesian domain only (not on a "
                                    "slab of a decomposed run, not on a SphericalPolar grid)");
        return PYROHIP_ERR_ARG;
    }
    r.ps = ps;
    r.pp = pp;
    r.ps_live0 = ps->cur;
    return 0;
}

int evolve_particles(EvolveRun &r)
{
    return r.ps ? particles_run_advance(r.ps, r.s, r.pp, r.d_scal, r.ps_live0) : 0;
}

int evolve_open(EvolveRun &r, pyrohip_state *s, const pyrohip_dt_policy *pol, double cfl, int cfl_kind, double cfl_a,
                double dx, double dy, int max_steps, bool global_min)
{
    pyrohip_ctx *c = s->ctx;
    r.s = s;
    r.max_steps = max_steps;
    r.cfl_kind = cfl_kind;
    r.cfl_par[0] = cfl_a; r.cfl_par[1] = dx; r.cfl_par[2] = dy;
    PYRO_TRY(evolve_begin(s, pol, cfl, dx, dy, max_steps, &r.H));
    r.d_scal = s->d_scal;
    const bool global = global_min && c->global_cfl;
    r.min_cached = cfl_min_cached(s, cfl_kind, cfl_a, dx, dy) && (!global || s->cfl_is_global);
    r.H.min0 = r.min_cached ? s->next_cfl_min : 0.0;
    r.H.keep0 = r.min_cached ? 1.0 : 0.0;
    PYRO_CHECK_HIP(hipMemcpyAsync(s->d_scal, &r.H, sizeof(r.H), hipMemcpyHostToDevice, c->stream));
    PYRO_CHECK_HIP(hipStreamSynchronize(c->stream));      // (pageable host memory: the copy has left r.H)
    if (global && c->comm != nullptr) {
        // decomposed run: all ranks keep their (global) minimum or none does -- a rank whose slab was written
        // since must reduce its array, and the others' kept minimum still counts that slab's OLD cells.  One
        // small all-reduce + read-back per call instead of a pass over the slab (0.9 ms at 2048 x 16384)
        PYRO_TRY(comm_allreduce_min_device(c, &s->d_scal->keep0));
        PYRO_CHECK_HIP(hipMemcpyAsync(c->reduce_host, &s->d_scal->keep0, sizeof(double), hipMemcpyDeviceToHost,
                                      c->stream));
        PYRO_CHECK_HIP(hipStreamSynchronize(c->stream));
        r.min_cached = ((double *)c->reduce_host)[0] == 1.0;
    }
    PYRO_CHECK_HIP(hipMemsetAsync(s->d_flag, 0, sizeof(int), c->stream));
    // (the bound set's error word sticks for the run)
    if (r.ps) PYRO_CHECK_HIP(hipMemsetAsync(r.ps->err, 0, sizeof(int), c->stream));
    s->pend_part = nullptr;
    return 0;
}

int evolve_fill(EvolveRun &r, bool frame, bool *frame_done)
{
    pyrohip_state *s = r.s;
    *frame_done = frame && frame_fill_ok(s, r.halo_ok, r.sph_ok);
    return *frame_done ? launch_frame(s, s->d, s->alt_base + geom_lead(s->g)) : pyrohip_fill_bc(s, -1);
}

int evolve_policy(EvolveRun &r, int m) { return launch_policy(r, m, 0, 1); }

int evolve_between(EvolveRun &r, int m, bool frame, bool fill, bool *frame_done)
{
    pyrohip_state *s = r.s;
    *frame_done = frame && frame_fill_ok(s, r.halo_ok, r.sph_ok);
    if (!*frame_done) {
        if (fill) PYRO_TRY(pyrohip_fill_bc(s, -1));
        return launch_policy(r, m, 0, 1);
    }
    const int npieces = frame_pieces(s->g);
    const auto kernel = s->nvar == 2 ? k_fill_frame2_policy<2> : k_fill_frame2_policy<4>;
    PYRO_LAUNCH(s->ctx, "k_fill_frame2_policy", kernel, dim3((npieces + 3) / 4 + 1),
                dim3(kPolicyThreads), 0, (const double *)s->d, s->d, s->alt_base + geom_lead(s->g), s->g,
                (const int *)s->d_bc, npieces, r.d_scal, r.dmin, (const int *)s->d_flag, s->d_dts, m, r.pend,
                r.npend, const_cast<double *>(r.dmin));
    PYRO_CHECK_HIP(hipGetLastError());
    r.pend = nullptr;
    return 0;
}

// A device-side run whose last iterations were inactive (past tmax, after an invalid state) has
// kept filling / copying ghost frames between the two buffers on those iterations: the frame of
// the buffer that holds the final state then depends on their parity -- rebuild it from the
// state before the last step that advanced (the other buffer: inactive launches store nothing).
static int restore_frame_after_inactive(pyrohip_state *s, int steps, int max_steps, bool halo_ok, bool sph_ok)
{
    if (steps < 1 || steps >= max_steps || !s->alt_base || !frame_fill_ok(s, halo_ok, sph_ok)) return 0;
    PYRO_TRY(launch_frame(s, s->alt_base + geom_lead(s->g), nullptr));
    PYRO_CHECK_HIP(hipStreamSynchronize(s->ctx->stream));
    return 0;
}

int evolve_close(EvolveRun &r, pyrohip_dt_policy *pol, int *steps_done, double *dts_out, bool framed,
                 bool one_launch)
{
    pyrohip_state *s = r.s;
    pyrohip_ctx *c = s->ctx;
    const Geom &g = s->g;
    const int max_steps = r.max_steps;
    // (one launch per step: every launch raises its own bit of the flag, by step parity)
    PYRO_TRY(launch_policy(r, max_steps, 1, one_launch ? (2 << ((max_steps - 1) & 1)) : 1));
    // the last step's halo exchange (posted on the halo stream) must have landed before
    // the call returns: the buffers may be read, written or freed by the caller next
    PYRO_TRY(comm_wait_halo(s));
    // the one round trip of the call: scalars, flag, last CFL minimum, the dt sequence
    char *hb = (char *)c->reduce_host;                       // 256 pinned bytes
    static_assert(sizeof(StepScalars) + 24 <= 256, "pinned scratch");
    PYRO_CHECK_HIP(hipMemcpyAsync(hb, r.d_scal, sizeof(StepScalars), hipMemcpyDeviceToHost, c->stream));
    PYRO_CHECK_HIP(hipMemcpyAsync(hb + sizeof(StepScalars), s->d_flag, sizeof(int), hipMemcpyDeviceToHost,
                                  c->stream));
    PYRO_CHECK_HIP(hipMemcpyAsync(hb + sizeof(StepScalars) + 8, r.dmin, sizeof(double), hipMemcpyDeviceToHost,
                                  c->stream));
    int *perr = (int *)(hb + sizeof(StepScalars) + 16);
    *perr = 0;
    if (r.ps)
        PYRO_CHECK_HIP(hipMemcpyAsync(perr, r.ps->err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (dts_out)
        PYRO_CHECK_HIP(hipMemcpyAsync(dts_out, s->d_dts, (size_t)max_steps * sizeof(double),
                                      hipMemcpyDeviceToHost, c->stream));
    PYRO_CHECK_HIP(hipStreamSynchronize(c->stream));
    StepScalars &H = r.H;
    memcpy(&H, hb, sizeof(H));
    // (a one-launch run raises per-launch bits of the flag; the policy keeps the verdict)
    const bool invalid = (*(int *)(hb + sizeof(StepScalars)) & 1) || H.dead;
    const double lastmin = *(double *)(hb + sizeof(StepScalars) + 8);
    // max_steps swaps were made; the last state that advanced sits H.steps swaps from the start
    if ((max_steps - H.steps) % 2) state_swap_alt(s);
    // the set: one exchange of its two buffers per step that advanced (a failing advance stored
    // nothing in the live one)
    const bool part_error = *perr != 0;
    if (r.ps) r.ps->cur ^= H.steps & 1;
    s->halo_pending = false;
    // the ghost frame of the final state: what single steps leave there is the filled frame of the
    // state BEFORE the last step that advanced, whose interior sits untouched in the other buffer
    if (one_launch) {
        // (its steps wrote no ghost cell; after an invalid step the other buffer is that step's
        // debris: the state's own images)
        if (H.steps >= 1) PYRO_TRY(launch_frame(s, invalid ? s->d : s->alt_base + geom_lead(g), nullptr));
    } else if (framed && !invalid && !r.own_frames) {
        PYRO_TRY(restore_frame_after_inactive(s, H.steps, max_steps, r.halo_ok, r.sph_ok));
    }
    // after an invalid step: the reference's assert fires right behind fill_BC_all (pyro_sim.py:250-256), so the
    // state left behind carries its own filled ghost cells -- whatever the step's launch and the inactive
    // iterations behind it did to the frames of the two buffers
    // (a stratified run: the fill in front of the step that met it is the last that wrote -- its fills keep
    // still on inactive iterations -- and that frame is the single steps'; another fill here would take the
    // hse corners from the momenta of THIS fill)
    if (invalid && !s->nb_set && !r.own_frames) PYRO_TRY(pyrohip_fill_bc(s, -1));
    // the minimum of the last launch belongs to the state only if that launch advanced it
    // (a stratified run ends with the interior's minimum alone: not kept, as after single steps)
    s->next_cfl_min = (H.steps == max_steps && !invalid && !r.own_frames) ? lastmin : -1.0;
    s->cfl_kind = r.cfl_kind;
    memcpy(s->cfl_par, r.cfl_par, sizeof(r.cfl_par));
    s->ghost_by_rules = false;      // a new time level: its ghost cells are stale until the next fill
    pol->t = H.t; pol->dt_old = H.dt_old; pol->n = H.n;
    *steps_done = H.steps;
    if (part_error) {
        set_error("a tracer particle's interpolation stencil leaves the state's array (position outside the "
                  "ghosted grid, NaN or infinite): the state and the particle set are those before that step");
        return PYROHIP_ERR_STATE;
    }
    if (invalid) {
        set_error("invalid state: min(rho) <= 0 or min(e) <= 0 on the interior "
                  "(compressible/simulation.py:68-71); the state is the one before that step");
        return PYROHIP_ERR_STATE;
    }
    return 0;
}

}  // namespace pyro
