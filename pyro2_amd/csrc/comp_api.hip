// extern "C" entry points of the compressible solver: argument checking and
// dispatch (PYRO_BUILD, builds.h) between the bit-faithful (exact) and contracted (fastm) builds
// of the compressible units.  What the units export is declared in comp_units.h: all of it in the
// bit-faithful build, in the contracted one the functions both builds define and no other.
#include "builds.h"
#include "common.h"
#include "stencil.h"

namespace pyro {
namespace exact {
#include "comp_units.h"
}
namespace fastm {
#define PYRO_UNITS_FAST 1
#include "comp_units.h"
}
}  // namespace pyro

using namespace pyro;

// "This call takes the row-marching wavefront kernel": kernel_set 2, or the library's choice
// (kernel_set -1) where that kernel fills the chip -- it needs >= ~2 wavefronts per SIMD of 56
// columns x >= 32 rows; measured crossover with the tile kernel at 2048^2 cells
// (profiles/r02_kernel_sets_by_size.txt).  SphericalPolar steps and the Runge-Kutta stages taken
// singly (pyrohip_comp_rk_rhs):
static bool takes_wave_kernel(const Geom &g, const pyrohip_comp_params *p)
{
    return p->kernel_set == 2 || (p->kernel_set == -1 && (double)g.nx * (double)g.ny >= 2048.0 * 2048.0);
}
// ... the Cartesian CTU step: in the contracted build from 1024^2 cells on with nx, ny >= 512 (round 6: with
// strips short enough for ONE round of resident wavefronts -- wave_rows down to 8 rows -- the row-marching
// kernel passes the tile kernel there: 1024^2 78.3 -> 71.0 us per step, 1152^2 90.9 -> 78.4, 1536^2 148.6 ->
// 136.6, 1792^2 190.4 -> 155.7; 896^2 a tie, below it and in the bit-faithful build the tile kernel stays ahead
// up to 2048^2: 1024^2 104.8 vs 114.6 us, 1536^2 203.5 vs 226.9)
// (a state with passive scalars, nvar > 4, steps on the tile kernel at every size)
static bool takes_wave_kernel_ctu(const Geom &g, const pyrohip_comp_params *p, int nvar = 4)
{
    if (nvar > 4) return false;
    const double cells = (double)g.nx * (double)g.ny;
    return p->kernel_set == 2 || (p->kernel_set == -1 && g.nx >= 512 && g.ny >= 512 &&
                                  cells >= (p->fast_math ? 1024.0 * 1024.0 : 2048.0 * 2048.0));
}

// All variables (the four hydro ones and the passive scalars) follow the same kind of index map on every side: outflow, reflect (even or
// odd), periodic -- or, where halo_ok, rows that arrived with a halo exchange (they are data).
// (they do for bc / bc_xodd / bc_yodd, simulation_null.py:72-112)
static bool same_index_map_kinds(const pyrohip_state *s, bool halo_ok)
{
    for (int sd = 0; sd < 4; sd++) {
        int kind0 = -1;
        for (int n = 0; n < s->nvar; n++) {
            const int b = s->bc[n * 4 + sd];
            const int kind = (b == PYROHIP_BC_OUTFLOW) ? 0
                             : (b == PYROHIP_BC_REFLECT_EVEN || b == PYROHIP_BC_REFLECT_ODD) ? 1
                             : (b == PYROHIP_BC_PERIODIC) ? 2
                             : (halo_ok && b == PYROHIP_BC_HALO) ? 3 : -1;
            if (kind < 0 || (n > 0 && kind != kind0)) return false;
            kind0 = kind;
        }
    }
    return true;
}

// May the tile kernel read the ghost cells through the boundary rules instead of from
// memory (pyrohip_comp_params.fuse_fill)?  Index maps exist for outflow / reflect /
// periodic sides (halo rows are data); the source terms read ghost cells of their own.
static bool comp_can_fuse_fill(const pyrohip_state *s, const pyrohip_comp_params *p, bool wave)
{
    if (wave || p->kernel_set == 0 || s->sph || s->user_bc || s->ramp_bc || s->ext_old ||
        p->grav != 0.0 || s->heat != nullptr)
        return false;
    return same_index_map_kinds(s, true);
}

// SphericalPolar grid: one launch (k_ctu_fused_sph) where the boundaries are index maps; the
// staged set (kernel_set 0: stage dumps) everywhere else
static bool comp_can_fuse_sph(const pyrohip_state *s, const pyrohip_comp_params *p)
{
    // (single domain; the tile kernel's 4-cell apron needs ng >= 4 and as many interior cells)
    if (!s->sph || p->kernel_set == 0 || s->nb_set || s->g.ng < 4 || s->g.nx < 4 || s->g.ny < 4 ||
        s->user_bc || s->ramp_bc || s->heat || s->ext_old || p->riemann != 1)
        return false;
    return same_index_map_kinds(s, false);
}

// Device-side stepping of a stratified state (hse / ambient y sides, the sponge):
// can k_fill_frame2_user fill its ghost frame?  Index maps on the x sides of every variable; index
// maps, hse or -- upper side -- ambient on the y sides; every image of a ghost cell an interior
// cell (nx, ny >= ng) and the cells at jlo and jhi two different ones.
static bool strat_fill_ok(const pyrohip_state *s)
{
    if (s->nvar != 4 || s->g.nx < s->g.ng || s->g.ny < s->g.ng || s->g.ny < 2) return false;
    for (int n = 0; n < 4; n++) {
        const int *b = &s->bc[n * 4];
        if (!bc_is_index_map(b[0], true) || !bc_is_index_map(b[1], true)) return false;
        if (!bc_is_index_map(b[2], true) && b[2] != PYROHIP_BC_HSE) return false;
        if (!bc_is_index_map(b[3], true) && b[3] != PYROHIP_BC_HSE && b[3] != PYROHIP_BC_AMBIENT) return false;
    }
    return true;
}

// max_scalars: passive scalars the entry point carries behind the four hydro planes (pyrohip_comp_step,
// pyrohip_comp_dt: 2; every other entry point: none)
static int check_comp(pyrohip_state *s, const pyrohip_comp_params *p, int max_scalars = 0)
{
    PYRO_REQUIRE(s && p, "NULL argument");
    if (max_scalars > 0)
        PYRO_REQUIRE(s->nvar >= 4 && s->nvar <= 4 + max_scalars,
                     "compressible state must have 4 variables (density, energy, x-momentum, y-momentum) "
                     "and at most 2 passive scalars behind them");
    else
        PYRO_REQUIRE(s->nvar == 4, "compressible state must have 4 variables "
                                   "(density, energy, x-momentum, y-momentum); passive scalars are "
                                   "carried by pyrohip_comp_step / pyrohip_comp_dt only");
    PYRO_REQUIRE(s->g.ng >= 4, "compressible needs ng >= 4 (compressible/simulation.py:194)");
    PYRO_REQUIRE(p->limiter >= 0 && p->limiter <= 2, "limiter must be 0, 1 or 2");
    PYRO_REQUIRE(p->dx > 0 && p->dy > 0 && p->gamma > 1.0, "bad dx/dy/gamma");
    return 0;
}

// The checks several entry points share.  fn: the caller's __func__ -- it opens the message, as in
// PYRO_REQUIRE, so the text that reaches Python names the entry point.  (check_sponge asks nothing
// where the sponge is off.)
static int require_in(const char *fn, bool cond, const char *msg)
{
    if (cond) return 0;
    set_error(std::string(fn) + ": " + msg);
    return PYROHIP_ERR_ARG;
}
static int check_riemann(const pyrohip_comp_params *p, const char *fn)
{
    return require_in(fn, p->riemann >= 0 && p->riemann <= 2, "riemann must be 0 (HLLC), 1 (CGF) or 2 (HLLC_lm)");
}
static int check_not_well_balanced(const pyrohip_comp_params *p, const char *fn)
{
    return require_in(fn, !p->well_balanced, "well_balanced is carried by pyrohip_comp_rk_rhs only (compressible_rk, "
                                             "stage by stage on the staged kernels)");
}
static int check_sponge(const pyrohip_comp_params *p, const char *fn)
{
    return require_in(fn, !p->do_sponge || p->sponge_rho_begin > p->sponge_rho_full,
                      "sponge_rho_begin must exceed sponge_rho_full (simulation.py:172)");
}

// What a state with passive scalars (planes 4, 5: partial densities rho X) excludes: they are carried
// by the tile kernel alone, with the upwinding of the HLLC solvers (the reference's CGF path cannot
// run with species: consFlux on an array of states does not broadcast, riemann.py:1163, 1177)
static int check_scalars(const pyrohip_state *s, const pyrohip_comp_params *p)
{
    if (s->nvar == 4) return 0;
    PYRO_REQUIRE(p->riemann != 1, "passive scalars: compressible.riemann = CGF is not carried "
                                  "(the reference cannot run it either); use HLLC or HLLC_lm");
    PYRO_REQUIRE(!s->sph, "passive scalars: SphericalPolar grids are not carried");
    PYRO_REQUIRE(!s->nb_set && !s->ctx->global_cfl, "passive scalars: decomposed runs (gpu.decompose, slabs) are not carried");
    PYRO_REQUIRE(!s->user_bc && !s->ramp_bc, "passive scalars: hse / ambient / ramp boundaries are not carried");
    PYRO_REQUIRE(!p->do_sponge, "passive scalars: the sponge (sponge.do_sponge) is not carried");
    PYRO_REQUIRE(!s->heat && !s->ext_old, "passive scalars: heating profiles and host-evaluated sources are not carried");
    PYRO_REQUIRE(p->kernel_set == 1 || p->kernel_set == -1,
                 "passive scalars: gpu.kernel_set 0 and 2 are not carried (the tile kernel, kernel_set 1, steps them)");
    PYRO_REQUIRE(s->g.nx >= 4 && s->g.ny >= 4, "passive scalars: the tile kernel needs at least 4 cells each way");
    for (size_t k = 0; k < s->bc.size(); k++)
        PYRO_REQUIRE(bc_is_index_map(s->bc[k], true),
                     "passive scalars: outflow / reflect / periodic boundaries only");
    return 0;
}

extern "C" {

// Up to max_steps iterations of the driver's loop without a host round trip per step: the run
// protocol of DESIGN.md 3.6.1 (evolve.hip) around the CTU step.  particles: a tracer set that
// rides along, or NULL.
int pyrohip_comp_evolve_p(pyrohip_state *s, const pyrohip_comp_params *p, double cfl,
                          pyrohip_dt_policy *pol, int max_steps, int *steps_done, double *dts_out,
                          pyrohip_particles *particles, const pyrohip_particle_params *pparams)
{
    PYRO_TRY(check_comp(s, p));
    PYRO_REQUIRE(pol && steps_done, "NULL argument");
    PYRO_REQUIRE(max_steps >= 1, "max_steps must be positive");
    PYRO_TRY(check_not_well_balanced(p, __func__));
    PYRO_REQUIRE(p->kernel_set != 0, "the staged kernel set steps from the host (kernel_set 0)");
    PYRO_TRY(check_riemann(p, __func__));
    // (a SphericalPolar grid steps on the device where its step is one launch: comp_can_fuse_sph)
    const bool sphf = s->sph != nullptr && comp_can_fuse_sph(s, p);
    PYRO_REQUIRE((!s->sph || sphf) && !s->ramp_bc && !s->ext_old,
                 "device-side stepping: no ramp boundary, no host-evaluated source; "
                 "a SphericalPolar grid needs CGF and outflow / reflect / periodic sides "
                 "(use pyrohip_comp_dt / pyrohip_comp_step)");
    pyrohip_ctx *c = s->ctx;
    // a stratified run: hse / ambient y sides and / or the sponge -- its own fill
    // (one launch, with the frame's CFL minimum) and the sponge behind every step
    const bool strat = s->user_bc || p->do_sponge != 0;
    if (strat) {
        PYRO_REQUIRE(!s->sph && !s->nb_set && !c->global_cfl && !particles && strat_fill_ok(s),
                     "device-side stepping: hse / ambient boundaries and the sponge step on the device on a "
                     "single Cartesian domain, without tracer particles: outflow / reflect / periodic x sides, "
                     "ambient on the upper y side only, at least ng cells each way "
                     "(use pyrohip_comp_dt / pyrohip_comp_step)");
        PYRO_REQUIRE(!s->user_bc || s->user_bc_set, "hse / ambient boundary: call pyrohip_state_set_user_bc first");
        PYRO_TRY(check_sponge(p, __func__));
    }
    const bool wave = !sphf && takes_wave_kernel_ctu(s->g, p);
    // SphericalPolar grid on the row-marching kernel (comp_sph_wave.hip: reads a filled frame)
    const bool sphw = sphf && takes_wave_kernel(s->g, p);
    const bool framed = wave || sphw;       // the step kernel works on filled ghost frames
    EvolveRun r;
    r.halo_ok = wave;       // (k_fill_frame2 along the halo rows of a slab; a SphericalPolar grid is a single domain)
    r.sph_ok = sphw;
    PYRO_TRY(evolve_bind_particles(r, s, particles, pparams, __func__));
    // (global_min: a decomposed run steps with the minimum over ALL slabs)
    PYRO_TRY(evolve_open(r, s, pol, cfl, 0, p->gamma, p->dx, p->dy, max_steps, true));
    double *fpart = nullptr, *spart = nullptr;
    int nfpart = 0, nspart = 0;
    if (strat) {
        // (a minimum a single step left is the interior's: the first step reduces the filled array)
        r.min_cached = false;
        r.own_frames = true;
        PYRO_TRY(state_alt(s));
        nfpart = PYRO_BUILD(p->fast_math, comp_fill_frame_user_parts(s));
        nspart = p->do_sponge ? PYRO_BUILD(p->fast_math, comp_sponge_run_parts(s)) : 0;
        PYRO_TRY(c->strat.ensure((size_t)(nfpart + nspart) * sizeof(double)));
        fpart = (double *)c->strat.p;
        spart = fpart + nfpart;
    }
    // steps after the first: the tile kernel applies the boundary rules itself where it can
    // (the first one needs filled ghost cells for the CFL minimum over the whole array)
    // (the spherical kernel reads every ghost cell through the boundary rules anyway)
    // (a stratified run always fills: the sponge acts on the ghost cells in memory)
    const bool fuse = !strat && ((sphf && !sphw) || comp_can_fuse_fill(s, p, wave));
    pyrohip_comp_params pf = *p;
    // step_launches 1: the row-marching kernel as the ONLY launch of a step (single domain;
    // outflow / reflect / periodic sides, the same kind for the four variables): it reads ghost
    // cells through the boundary rules instead of a filled frame, and every wavefront derives
    // the step's dt from the CFL minima the previous launch left (k_ctu_wave<.., ONE>, common.h:
    // StepPolicy).  The first step keeps its fill + CFL + policy launches (the CFL minimum of
    // the state as handed over), the closing policy call is a launch, and the ghost cells of
    // the final state are filled once at the end.  Bit-identical to the three launches, and
    // measured no faster (profiles/r04_one_launch_step.txt: every wavefront of that instance starts
    // with ~5 us of dependent latency, the two small launches cost 1-2.5 % of a step; -1.5 % at
    // 16384^2): not the default.
    // (with a particle set bound the run keeps the three launches: the one-launch steps write no ghost
    // cell, and the tracers within half a cell of an upper border read the new buffer's frame)
    bool one_launch = !strat && wave && p->step_launches == 1 && !s->nb_set && !c->global_cfl && !r.ps &&
                      comp_can_fuse_fill(s, p, false);
    for (int k = 0; k < 16 && one_launch; k++) one_launch = (s->bc[k] != PYROHIP_BC_HALO);
    pyro::StepPolicy *d_pol = nullptr;
    if (one_launch) {
        // three sets of slots (+inf), the reduced minimum, then the StepPolicy of this call
        using namespace pyro;
        const size_t nw = 3 * (size_t)kPolSetWords + 1;
        const size_t bytes = nw * 8 + sizeof(StepPolicy);
        if (!s->d_polmem) PYRO_CHECK_HIP(hipMalloc((void **)&s->d_polmem, bytes));
        std::vector<unsigned long long> init(nw + (sizeof(StepPolicy) + 7) / 8, 0ull);
        const double inf = INFINITY;
        for (size_t k = 0; k < nw; k++) memcpy(&init[k], &inf, 8);
        StepPolicy sp;
        memset(&sp, 0, sizeof(sp));
        sp.S[0] = r.H;
        sp.slots = s->d_polmem;
        sp.dts = s->d_dts;
        memcpy(&init[nw], &sp, sizeof(sp));
        PYRO_CHECK_HIP(hipMemcpy(s->d_polmem, init.data(), bytes, hipMemcpyHostToDevice));
        d_pol = (StepPolicy *)(s->d_polmem + nw);
        r.d_scal = &d_pol->S[0];    // (the step scalars of a one-launch run: two copies, by step parity)
    }
    int rc = 0;
    for (int m = 0; m < max_steps && rc == 0; m++) {
        if (one_launch && m > 0) {
            s->pol_next = d_pol;
            s->pol_m = m;
            rc = PYRO_BUILD(p->fast_math, comp_step_wave_ex(s, p, 0.0, r.d_scal, &r.dmin));
            continue;
        }
        // ghost cells: halos of a slab first, then the boundary fill (pyro_sim.py:250-256)
        if (s->nb_set && c->comm != nullptr) rc = pyrohip_halo_exchange(s, s->nb_lo, s->nb_hi);
        if (rc) break;
        pf.fuse_fill = (fuse && m > 0) ? 1 : 0;
        bool frame_done = false;
        if (strat) {
            // one launch: the frames of both buffers by the hse / ambient rules and the CFL partials
            // of the cells written; nothing on an iteration that will not advance
            rc = PYRO_BUILD(p->fast_math, comp_fill_frame_user(s, p, r.d_scal, fpart));
            if (rc) break;
            frame_done = true;
            if (m == 0) {   // CFL minimum of the state as handed over: the full reduction
                rc = PYRO_BUILD(p->fast_math, comp_cfl_min_device(s, p, &r.dmin));
                if (rc) break;
            } else {        // min(interior: the last step's or the sponge's partials, frame: the fill's)
                r.fpart = fpart;
                r.nfpart = nfpart;
            }
            rc = evolve_policy(r, m);
        } else if (m == 0) {   // CFL minimum of the state as handed over (full array, ghost cells filled)
            rc = evolve_fill(r, framed, &frame_done);
            if (rc) break;
            if (r.min_cached)
                r.dmin = &r.d_scal->min0;      // (... the one the previous call's last step left)
            else if (sphf)
                rc = PYRO_BUILD(p->fast_math, comp_cfl_min_device_sph(s, p, &r.dmin));
            else
                rc = PYRO_BUILD(p->fast_math, comp_cfl_min_device(s, p, &r.dmin));
            if (rc) break;
            // decomposed run: every rank steps with the minimum over ALL slabs -- also in the
            // first step of a call (found by running four ranks on one GPU: the slabs far from
            // the blast started every call with their own, larger dt; with two ranks the two
            // local minima are equal by symmetry and nothing showed)
            // (a kept minimum is the global one already: every rank kept it, evolve_open)
            if (c->global_cfl && !r.min_cached) {
                rc = comm_allreduce_min_device(c, const_cast<double *>(r.dmin));
                if (rc) break;
                s->cfl_is_global = true;
            }
            rc = evolve_policy(r, 0);
        } else
            rc = evolve_between(r, m, framed, !pf.fuse_fill, &frame_done);
        if (rc) break;
        s->frame_prefilled = frame_done;
        s->next_cfl_min = 1.0;      // "cached on the device": keeps a posted halo exchange valid
        s->cfl_kind = 0;
        s->pol_next = d_pol;    // (one launch per step: this is step 0, its dt is in S[0])
        s->pol_m = 0;
        if (sphw)
            rc = PYRO_BUILD(p->fast_math, comp_step_wave_sph_ex(s, &pf, 0.0, r.d_scal, &r.dmin));
        else if (sphf)
            rc = PYRO_BUILD(p->fast_math, comp_step_fused_sph_ex(s, &pf, 0.0, r.d_scal, &r.dmin));
        else if (wave)
            rc = PYRO_BUILD(p->fast_math, comp_step_wave_ex(s, p, 0.0, r.d_scal, &r.dmin));
        else
            rc = PYRO_BUILD(p->fast_math, comp_step_fused_ex(s, &pf, 0.0, r.d_scal, &r.dmin));
        r.take_pending();       // (the minimum of a tile-kernel launch is taken by the next policy call)
        if (rc == 0 && p->do_sponge) {
            // the sponge on the new buffer, ghost frame included; the next policy call takes the
            // partials of the interior behind it, not the step's
            rc = PYRO_BUILD(p->fast_math, comp_sponge_run(s, p, r.d_scal, spart));
            r.pend = spart;
            r.npend = nspart;
        }
        if (rc == 0) rc = evolve_particles(r);
    }
    s->frame_prefilled = false;      // (an iteration that stopped between the fill and its step)
    s->pol_next = nullptr;
    PYRO_TRY(rc);
    if (one_launch) {
        // the closing policy call: on the scalars of the last step's parity, with the minimum of the
        // slots the last launch filled -- unused words hold +inf
        r.d_scal = &d_pol->S[(max_steps - 1) & 1];
        r.pend = (const double *)(s->d_polmem + (size_t)((max_steps - 1) % 3) * pyro::kPolSetWords);
        r.npend = pyro::kPolSetWords;
        r.dmin = (const double *)(s->d_polmem + 3 * (size_t)pyro::kPolSetWords);
    }
    rc = evolve_close(r, pol, steps_done, dts_out, framed && !strat, one_launch);
    if (s->next_cfl_min <= 0.0) s->cfl_is_global = false;
    return rc;
}

int pyrohip_comp_evolve(pyrohip_state *s, const pyrohip_comp_params *p, double cfl,
                        pyrohip_dt_policy *pol, int max_steps, int *steps_done, double *dts_out)
{
    return pyrohip_comp_evolve_p(s, p, cfl, pol, max_steps, steps_done, dts_out, nullptr, nullptr);
}

// An ensemble of independent runs on one grid, stepped together: per iteration ONE
// policy launch (a workgroup per member) and ONE launch of the tile kernel (blockIdx.y = member) for
// all of them.  What pyrohip_comp_evolve does for a single run on the tile kernel, member by member:
// the same first iteration with the existing launches, the same close.
int pyrohip_comp_evolve_batch(pyrohip_state *const *members, int nmembers, const pyrohip_comp_params *p, double cfl,
                              pyrohip_dt_policy *pols, int max_steps, int *steps_done, double *dts_out, int *status)
{
    const char *fn = "batch";
    PYRO_TRY(require_in(fn, members && p && pols && steps_done && status, "NULL argument"));
    PYRO_TRY(require_in(fn, nmembers >= 1 && nmembers <= 65535, "1 to 65535 members"));
    PYRO_TRY(require_in(fn, max_steps >= 1, "max_steps must be positive"));
    for (int m = 0; m < nmembers; m++) PYRO_TRY(require_in(fn, members[m] != nullptr, "a member is NULL"));
    pyrohip_state *s0 = members[0];
    pyrohip_ctx *c = s0->ctx;
    for (int m = 0; m < nmembers; m++) {
        const pyrohip_state *s = members[m];
        const std::string who = "member " + std::to_string(m) + ": ";
        PYRO_TRY(require_in(fn, s->ctx == c, (who + "another context than member 0's").c_str()));
        PYRO_TRY(require_in(fn, s->nvar == 4, (who + "nvar must be 4 (density, energy, x-momentum, y-momentum; "
                                                     "passive scalars are not carried)").c_str()));
        PYRO_TRY(require_in(fn, s->g.nx == s0->g.nx && s->g.ny == s0->g.ny,
                            (who + "another shape (nx, ny) than member 0's").c_str()));
        PYRO_TRY(require_in(fn, s->g.ng == s0->g.ng, (who + "another ng than member 0's").c_str()));
        PYRO_TRY(require_in(fn, s->bc == s0->bc, (who + "other boundary codes than member 0's").c_str()));
        for (int k = 0; k < m; k++)
            PYRO_TRY(require_in(fn, members[k] != s, (who + "the same state is listed twice").c_str()));
        // what the tile kernel with the ghost fill folded in does not carry (comp_can_fuse_fill), by name
        PYRO_TRY(require_in(fn, !s->sph, (who + "SphericalPolar grids are not carried").c_str()));
        PYRO_TRY(require_in(fn, !s->user_bc && !s->ramp_bc,
                            (who + "hse / ambient / ramp sides are not carried").c_str()));
        PYRO_TRY(require_in(fn, !s->heat, (who + "a heating profile is not carried").c_str()));
        PYRO_TRY(require_in(fn, !s->ext_old && !s->ext_new, (who + "host-evaluated sources are not carried").c_str()));
        PYRO_TRY(require_in(fn, !s->nb_set, (who + "slabs of a decomposed run are not carried").c_str()));
    }
    PYRO_TRY(require_in(fn, !c->global_cfl, "a global CFL minimum (decomposed runs) is not carried"));
    PYRO_TRY(require_in(fn, s0->g.nx >= 4 && s0->g.ny >= 4, "the tile kernel needs at least 4 cells in each direction"));
    PYRO_TRY(require_in(fn, s0->g.ng >= 4, "compressible needs ng >= 4 (compressible/simulation.py:194)"));
    PYRO_TRY(require_in(fn, same_index_map_kinds(s0, false),
                        "outflow / reflect / periodic sides only, the same kind for the four variables"));
    PYRO_TRY(require_in(fn, p->limiter >= 0 && p->limiter <= 2, "limiter must be 0, 1 or 2"));
    PYRO_TRY(require_in(fn, p->dx > 0 && p->dy > 0 && p->gamma > 1.0, "bad dx/dy/gamma"));
    PYRO_TRY(check_riemann(p, fn));
    PYRO_TRY(require_in(fn, p->grav == 0.0, "gravity (grav != 0) is not carried"));
    PYRO_TRY(require_in(fn, !p->do_sponge, "the sponge (do_sponge) is not carried"));
    PYRO_TRY(require_in(fn, !p->well_balanced, "well_balanced is not carried"));
    PYRO_TRY(require_in(fn, p->kernel_set == -1 || p->kernel_set == 1,
                        "kernel_set 0 and 2 are not carried (the tile kernel, kernel_set 1 or -1, steps an ensemble)"));

    // context scratch: the table | scalars, minima, flags, dt sequences (ONE read-back) | CFL partials
    const int N = nmembers, nt = PYRO_BUILD(p->fast_math, comp_fused_tiles(s0));
    const size_t o_scal = (size_t)N * sizeof(BatchMember), o_min = o_scal + (size_t)N * sizeof(StepScalars),
                 o_flag = o_min + (size_t)N * 8, o_dts = o_flag + (((size_t)N * 4 + 7) & ~(size_t)7),
                 o_part = o_dts + (size_t)N * (max_steps + 1) * 8, total = o_part + (size_t)N * nt * 8;
    static_assert(sizeof(BatchMember) % 8 == 0 && sizeof(StepScalars) % 8 == 0, "8-byte fields");
    PYRO_TRY(c->batch.ensure(total));
    char *db = (char *)c->batch.p;
    std::vector<char> hb(o_part, 0);
    BatchMember *tab = (BatchMember *)hb.data();
    StepScalars *H = (StepScalars *)(hb.data() + o_scal);
    std::vector<char> cached(N, 0);
    for (int m = 0; m < N; m++) {
        pyrohip_state *s = members[m];
        PYRO_TRY(comm_wait_halo(s));
        PYRO_TRY(state_alt(s));
        BatchMember &M = tab[m];
        memset(&M, 0, sizeof(M));
        set_member_ptr(M.buf[0], s->d);
        set_member_ptr(M.buf[1], s->alt_base + geom_lead(s->g));
        set_member_ptr(M.S, (StepScalars *)(db + o_scal) + m);
        set_member_ptr(M.minout, (double *)(db + o_min) + m);
        set_member_ptr(M.flag, (int *)(db + o_flag) + m);
        set_member_ptr(M.dts, (double *)(db + o_dts) + (size_t)m * (max_steps + 1));
        set_member_ptr(M.part, (double *)(db + o_part) + (size_t)m * nt);
        evolve_scalars(&pols[m], cfl, p->dx, p->dy, &H[m]);
        // the minimum the member's last call left still describes it (evolve_open)
        cached[m] = cfl_min_cached(s, 0, p->gamma, p->dx, p->dy) ? 1 : 0;
        H[m].min0 = cached[m] ? s->next_cfl_min : 0.0;
        H[m].keep0 = cached[m] ? 1.0 : 0.0;
        s->pend_part = nullptr;
    }
    PYRO_CHECK_HIP(hipMemcpyAsync(db, hb.data(), o_part, hipMemcpyHostToDevice, c->stream));
    PYRO_CHECK_HIP(hipStreamSynchronize(c->stream));      // (pageable host memory: the copy has left hb)
    const BatchMember *d_tab = (const BatchMember *)db;
    // A launch or copy that fails from here on leaves work enqueued on members whose buffers may have changed
    // places an unknown number of times: the error is collected, and before it is returned every member is
    // put into a state the other entry points can work on (contents undefined, nothing cached, ghost cells stale)
    const auto abandon = [&](int rc) {
        (void)hipStreamSynchronize(c->stream);
        for (int m = 0; m < N; m++) {
            pyrohip_state *s = members[m];
            s->halo_pending = false;
            s->frame_prefilled = false;
            s->ghost_by_rules = false;
            s->next_cfl_min = -1.0;
            s->cfl_is_global = false;
            steps_done[m] = 0;
            status[m] = 0;
        }
        return rc;
    };
    int rc = 0;
    // first iteration, member by member with the launches of a single run: ghost fill, the CFL minimum
    // of the filled array (or the kept one), the policy
    for (int m = 0; m < N && rc == 0; m++) {
        pyrohip_state *s = members[m];
        rc = pyrohip_fill_bc(s, -1);
        const double *dmin = &member_ptr(tab[m].S)->min0;
        if (rc == 0 && !cached[m]) rc = PYRO_BUILD(p->fast_math, comp_cfl_min_device(s, p, &dmin));
        if (rc == 0) rc = evolve_batch_policy0(c, tab[m], dmin);
    }
    for (int it = 0; it < max_steps && rc == 0; it++) {
        if (it > 0) rc = evolve_batch_policy(c, d_tab, N, nt, it, 0);
        if (rc == 0) rc = PYRO_BUILD(p->fast_math, comp_step_fused_batch(s0, p, d_tab, N, it & 1));
    }
    if (rc == 0) rc = evolve_batch_policy(c, d_tab, N, nt, max_steps, 1);
    // the one round trip of the call
    if (rc == 0)
        rc = (int)hipMemcpyAsync(hb.data() + o_scal, db + o_scal, o_part - o_scal, hipMemcpyDeviceToHost, c->stream);
    if (rc == 0) {
        rc = (int)hipStreamSynchronize(c->stream);
        if (rc != 0) set_error(std::string("batch: the read-back failed: ") + hipGetErrorString((hipError_t)rc));
    }
    if (rc != 0) return abandon(rc);
    // the close, member by member as evolve_close does it for a run on the tile kernel
    const double *mins = (const double *)(hb.data() + o_min);
    const int *flags = (const int *)(hb.data() + o_flag);
    const double *dts = (const double *)(hb.data() + o_dts);
    for (int m = 0; m < N; m++) {
        pyrohip_state *s = members[m];
        const StepScalars &R = H[m];
        const bool invalid = (flags[m] & 1) || R.dead;
        // every iteration exchanged the member's buffers, the first R.steps of them advanced it: the
        // last state that advanced (after an invalid step: the one before it) sits R.steps exchanges on
        if (R.steps % 2) state_swap_alt(s);
        s->halo_pending = false;
        s->frame_prefilled = false;
        s->ghost_by_rules = false;      // a new time level: its ghost cells are stale until the next fill
        // after an invalid step the state carries its own filled ghost cells (evolve_close)
        if (invalid) PYRO_TRY(pyrohip_fill_bc(s, -1));
        // the minimum of the last launch belongs to the state only if that launch advanced it
        s->next_cfl_min = (R.steps == max_steps && !invalid) ? mins[m] : -1.0;
        s->cfl_is_global = false;
        s->cfl_kind = 0;
        s->cfl_par[0] = p->gamma; s->cfl_par[1] = p->dx; s->cfl_par[2] = p->dy;
        pols[m].t = R.t; pols[m].dt_old = R.dt_old; pols[m].n = R.n;
        steps_done[m] = R.steps;
        status[m] = invalid ? PYROHIP_ERR_STATE : 0;
        if (dts_out)
            memcpy(dts_out + (size_t)m * max_steps, dts + (size_t)m * (max_steps + 1), (size_t)max_steps * sizeof(double));
    }
    return 0;
}

int pyrohip_comp_dt(pyrohip_state *s, const pyrohip_comp_params *p, double cfl, double *dt_out)
{
    PYRO_TRY(check_comp(s, p, 2));      // (the CFL minimum reads the four hydro planes)
    PYRO_REQUIRE(dt_out, "dt_out is NULL");
    if (s->sph) {
        // (cached by the one-launch spherical step: whole-array minimum of the new state; every
        // other path that touches the state, the staged spherical set included, resets it)
        if (s->next_cfl_min > 0.0 && s->cfl_kind == 0) { *dt_out = cfl * s->next_cfl_min; return 0; }
        return PYRO_BUILD(p->fast_math, comp_dt_sph(s, p, cfl, dt_out));
    }
    return PYRO_BUILD(p->fast_math, comp_dt(s, p, cfl, dt_out));
}

int pyrohip_comp_dt_is_cached(pyrohip_state *s, int *flag)
{
    PYRO_REQUIRE(s && flag, "NULL argument");
    *flag = (s->next_cfl_min > 0.0 && s->cfl_kind == 0 && !s->user_bc && !s->ramp_bc) ? 1 : 0;
    return 0;
}

int pyrohip_comp_rk_dt_is_cached(pyrohip_state *s, int *flag)
{
    PYRO_REQUIRE(s && flag, "NULL argument");
    *flag = (s->next_cfl_min > 0.0 && s->cfl_kind == 1) ? 1 : 0;
    return 0;
}

int pyrohip_comp_dt_is_global(pyrohip_state *s, int *flag)
{
    PYRO_REQUIRE(s && flag, "NULL argument");
    *flag = (s->next_cfl_min > 0.0 && s->cfl_kind == 0 && s->cfl_is_global && !s->user_bc && !s->ramp_bc) ? 1 : 0;
    return 0;
}

int pyrohip_comp_step(pyrohip_state *s, const pyrohip_comp_params *p, double dt)
{
    PYRO_TRY(check_comp(s, p, 2));
    PYRO_REQUIRE(dt > 0.0, "dt must be positive");
    PYRO_TRY(check_not_well_balanced(p, __func__));
    PYRO_REQUIRE(p->kernel_set >= -1 && p->kernel_set <= 2, "kernel_set must be -1 (automatic), 0, 1 or 2");
    PYRO_TRY(check_riemann(p, __func__));
    int rc;
    PYRO_REQUIRE(!s->ext_pending, "the corrector of the host-evaluated source has not run "
                                  "(pyrohip_comp_source_correct)");
    PYRO_TRY(check_scalars(s, p));
    pyrohip_comp_params pf = *p;
    if (p->fuse_fill) {
        // ghost cells not filled by the caller: folded into the tile kernel where that
        // works, the ordinary fill first everywhere else
        // (the spherical one-launch kernel reads every ghost cell through the boundary rules)
        const bool wave = !s->sph && takes_wave_kernel_ctu(s->g, p, s->nvar);
        if (!comp_can_fuse_fill(s, p, wave) && !comp_can_fuse_sph(s, p)) {
            PYRO_TRY(pyrohip_fill_bc(s, -1));
            pf.fuse_fill = 0;
        }
        p = &pf;
    }
    if (s->sph) {
        // compressible/simulation.py:206-208: no HLLC on a SphericalPolar grid
        PYRO_REQUIRE(p->riemann == 1, "a SphericalPolar grid needs the CGF Riemann solver");
        PYRO_REQUIRE(!s->user_bc && !s->ramp_bc && !s->heat && !s->ext_old,
                     "hse / ambient / ramp boundaries and heating are Cartesian-only");
        // the one-launch kernel reads EVERY ghost cell through the boundary rules: only where the
        // ghost cells are known to be those images -- the caller left the fill to the kernel, or the
        // last thing that wrote the state was the library's own full fill.  Ghost cells a host-side
        // boundary callback wrote (uploaded afterwards) are read from memory by the staged set.
        const bool fuse_sph = comp_can_fuse_sph(s, p) && (p->fuse_fill || s->ghost_by_rules);
        if (fuse_sph && takes_wave_kernel(s->g, p)) {
            // the row-marching kernel reads the state's ghost cells from memory: filled here if
            // the caller left the fill to the step
            if (p->fuse_fill) PYRO_TRY(pyrohip_fill_bc(s, -1));
            rc = PYRO_BUILD(p->fast_math, comp_step_wave_sph(s, p, dt));
        } else if (fuse_sph)
            rc = PYRO_BUILD(p->fast_math, comp_step_fused_sph(s, p, dt));
        else
            rc = PYRO_BUILD(p->fast_math, comp_step_sph(s, p, dt));
    } else if (s->ext_old) {
        // host-evaluated source: staged kernels up to the predictor U* = U + dt S(U^n);
        // the caller evaluates S_h(U*) and finishes with pyrohip_comp_source_correct
        PYRO_REQUIRE(!s->heat && !s->ramp_bc, "a host-evaluated source excludes the heating "
                     "profile and the ramp boundary (which zeroes the source arrays, BC.py:198-200)");
        return PYRO_BUILD(p->fast_math, comp_step_staged(s, p, dt));
    } else if (takes_wave_kernel_ctu(s->g, p, s->nvar))
        rc = PYRO_BUILD(p->fast_math, comp_step_wave(s, p, dt));
    else if (p->kernel_set == 1 || p->kernel_set == -1)
        rc = PYRO_BUILD(p->fast_math, comp_step_fused(s, p, dt));
    else
        rc = PYRO_BUILD(p->fast_math, comp_step_staged(s, p, dt));
    s->ghost_by_rules = false;      // a new time level: its ghost cells are stale until the next fill
    if (rc == 0 && p->do_sponge) {
        PYRO_TRY(check_sponge(p, __func__));
        rc = exact::comp_sponge(s, p, dt);
    }
    return rc;
}

int pyrohip_state_set_source(pyrohip_state *s, int which, pyrohip_state *src)
{
    PYRO_REQUIRE(s && (which == 0 || which == 1), "NULL state / which must be 0 (old) or 1 (new)");
    if (src) {
        PYRO_REQUIRE(src->nvar == 4 && s->nvar == 4 && src->g.nx == s->g.nx &&
                     src->g.ny == s->g.ny && src->g.ng == s->g.ng && src->ctx == s->ctx,
                     "the source state must match the 4-variable state it acts on");
    }
    if (which == 0) {
        PYRO_REQUIRE(!s->ext_pending, "the corrector of the previous step has not run");
        s->ext_old = src ? src->d : nullptr;
    } else {
        s->ext_new = src ? src->d : nullptr;
    }
    return 0;
}

int pyrohip_comp_source_correct(pyrohip_state *s, const pyrohip_comp_params *p, double dt)
{
    PYRO_TRY(check_comp(s, p));
    PYRO_REQUIRE(s->ext_pending && s->ext_old && s->ext_new,
                 "needs a predictor step (pyrohip_comp_step with a source set) and S_h(U*)");
    int rc = exact::comp_source_correct(s, p, dt);
    if (rc == 0 && p->do_sponge) {
        PYRO_TRY(check_sponge(p, __func__));
        rc = exact::comp_sponge(s, p, dt);
    }
    return rc;
}

int pyrohip_comp_rk_dt(pyrohip_state *s, const pyrohip_comp_params *p, double cfl, double *dt_out)
{
    PYRO_TRY(check_comp(s, p));
    PYRO_REQUIRE(dt_out, "dt_out is NULL");
    // (left by the last stage of pyrohip_comp_rk_step: the minimum over the new interior, which
    // is the whole-array minimum of simulation.py:46-56 once the ghost cells are images)
    if (s->next_cfl_min > 0.0 && s->cfl_kind == 1) { *dt_out = cfl * s->next_cfl_min; return 0; }
    return exact::comp_rk_dt(s, p, cfl, dt_out);
}

// ... the whole Runge-Kutta step (pyrohip_comp_rk_step / _evolve): kernel_set 2, or the library's
// choice from the size on at which the row-marching kernel passes the stage tile kernel.  Measured,
// the RK4 step alone on Sedov (profiles/comprk_tile_time.txt; row-marching / tile): contracted build
// 512^2 1.43, 768^2 1.17, 896^2 1.03 (a tie), 1024^2 0.87, 1536^2 0.79, 2048^2 0.74, 4096^2 0.68;
// bit-faithful build 512^2 1.84, 1024^2 1.14, 1536^2 1.08, 2048^2 1.03, 3072^2 1.01 (a tie: the
// row-marching kernel keeps it), 4096^2 0.96.
static bool takes_wave_kernel_rk(const Geom &g, const pyrohip_comp_params *p)
{
    const double side = p->fast_math ? 1024.0 : 3072.0;
    return p->kernel_set == 2 || (p->kernel_set == -1 && (double)g.nx * (double)g.ny >= side * side);
}
// "This Runge-Kutta step takes the stage tile kernel" (comp_rk_tile.hip): where the row-marching
// kernel does not take the call, with kernel_set 1 or the library's choice, on a grid whose ghost
// images are interior cells (4 cells each way).  kernel_set 0 stays staged (stage dumps).
static bool takes_rk_tile(const Geom &g, const pyrohip_comp_params *p)
{
    return !takes_wave_kernel_rk(g, p) && (p->kernel_set == -1 || p->kernel_set == 1) && g.nx >= 4 && g.ny >= 4;
}

// The whole Runge-Kutta step in nstages launches of ONE kernel -- the row-marching kernel
// (comp_wave.hip: comp_rk_step_wave) where the call takes it (takes_wave_kernel_rk), the stage tile
// kernel (comp_rk_tile.hip: comp_rk_step_tile) below that size and with kernel_set 1?  Single
// Cartesian domain, outflow / reflect / periodic sides (the same kind for the four variables: the
// stage states' ghost cells are read through index maps), no sponge, no heating profile, no
// host-evaluated source, no well-balanced reconstruction (neither kernel carries them).
static bool comp_rk_can_fuse(const pyrohip_state *y, const pyrohip_comp_params *p, const pyrohip_state *k,
                             int nstages)
{
    if (y->nvar != 4 || y->sph || y->nb_set || y->user_bc || y->ramp_bc || y->heat || y->ext_old ||
        p->do_sponge || p->well_balanced || y->g.ng < 4 || nstages < 2 || nstages > 4 || !k || k->nvar < 4 * nstages)
        return false;
    return (takes_wave_kernel_rk(y->g, p) || takes_rk_tile(y->g, p)) && same_index_map_kinds(y, false);
}

// the step itself, by the same predicate
static int comp_rk_step_any(pyrohip_state *y, const pyrohip_comp_params *p, pyrohip_state *k, int nstages,
                            const double *a, const double *b, double dt, const StepScalars *S, const double **dmin)
{
    if (takes_wave_kernel_rk(y->g, p))
        return PYRO_BUILD(p->fast_math, comp_rk_step_wave(y, p, k, nstages, a, b, dt, S, dmin));
    return PYRO_BUILD(p->fast_math, comp_rk_step_tile(y, p, k, nstages, a, b, dt, S, dmin));
}

// The first iteration of a method-of-lines run (pyrohip_comp_rk_evolve_p, fv4_run): the CFL minimum of
// the state as handed over -- whole array, ghost cells filled -- or the one the previous call's last
// stage left, then the dt policy
static int rk_first_iteration(EvolveRun &r, pyrohip_state *s, const pyrohip_comp_params *p, bool *frame_done)
{
    int rc = evolve_fill(r, false, frame_done);
    if (r.min_cached) r.dmin = &s->d_scal->min0;
    else if (rc == 0) rc = exact::comp_rk_cfl_min_device(s, p, &r.dmin);
    if (rc == 0) rc = evolve_policy(r, 0);
    return rc;
}

static int check_rk(pyrohip_state *y, const pyrohip_comp_params *p, pyrohip_state *k, int nstages,
                    const double *a, const double *b)
{
    PYRO_TRY(check_comp(y, p));
    PYRO_REQUIRE(k && a && b && k->ctx == y->ctx, "NULL argument / k state on another context");
    PYRO_REQUIRE(nstages >= 2 && nstages <= 4, "2 to 4 stages (RK2, TVD2, TVD3, RK4)");
    PYRO_REQUIRE(k->g.nx == y->g.nx && k->g.ny == y->g.ny && k->g.ng == y->g.ng && k->nvar >= 4 * nstages,
                 "the k state must have the geometry of the state and 4 planes per stage");
    PYRO_TRY(check_riemann(p, __func__));
    for (int s = 0; s < nstages; s++)
        for (int j = s; j < nstages; j++)
            PYRO_REQUIRE(a[s * nstages + j] == 0.0, "explicit methods only (strictly lower triangular a)");
    return 0;
}

int pyrohip_comp_rk_can_fuse(pyrohip_state *y, const pyrohip_comp_params *p, pyrohip_state *k, int nstages,
                             int *flag)
{
    PYRO_REQUIRE(y && p && flag, "NULL argument");
    *flag = comp_rk_can_fuse(y, p, k, nstages) ? 1 : 0;
    return 0;
}

int pyrohip_comp_rk_step(pyrohip_state *y, const pyrohip_comp_params *p, pyrohip_state *k, double dt,
                         int nstages, const double *a, const double *b)
{
    PYRO_TRY(check_rk(y, p, k, nstages, a, b));
    PYRO_REQUIRE(dt > 0.0, "dt must be positive");
    PYRO_TRY(check_not_well_balanced(p, __func__));
    PYRO_REQUIRE(comp_rk_can_fuse(y, p, k, nstages),
                 "pyrohip_comp_rk_step: single Cartesian domain, outflow / reflect / periodic sides, no sponge / "
                 "heating / host source, kernel_set -1, 1 or 2 and at least 4 cells each way "
                 "(pyrohip_comp_rk_can_fuse; otherwise stage by stage: pyrohip_comp_rk_rhs + pyrohip_state_lincomb)");
    const int rc = comp_rk_step_any(y, p, k, nstages, a, b, dt, nullptr, nullptr);
    y->ghost_by_rules = false;
    return rc;
}

// Up to max_steps steps of the compressible_rk driver loop (pyro_sim.py:241-281 with
// compressible_rk/simulation.py:46-104) without a host round trip per step: as pyrohip_comp_evolve,
// with the Runge-Kutta step above between the policy calls.
int pyrohip_comp_rk_evolve_p(pyrohip_state *y, const pyrohip_comp_params *p, pyrohip_state *k, int nstages,
                             const double *a, const double *b, double cfl, pyrohip_dt_policy *pol,
                             int max_steps, int *steps_done, double *dts_out, pyrohip_particles *particles,
                             const pyrohip_particle_params *pparams)
{
    PYRO_TRY(check_rk(y, p, k, nstages, a, b));
    PYRO_REQUIRE(pol && steps_done && max_steps >= 1, "NULL argument / max_steps must be positive");
    PYRO_TRY(check_not_well_balanced(p, __func__));
    PYRO_REQUIRE(comp_rk_can_fuse(y, p, k, nstages),
                 "device-side stepping: compressible_rk needs the conditions of pyrohip_comp_rk_step "
                 "(pyrohip_comp_rk_can_fuse)");
    pyrohip_state *s = y;
    pyrohip_ctx *c = s->ctx;
    PYRO_REQUIRE(!c->global_cfl, "device-side stepping: compressible_rk runs on a single domain");
    EvolveRun r;
    PYRO_TRY(evolve_bind_particles(r, s, particles, pparams, __func__));
    PYRO_TRY(evolve_open(r, s, pol, cfl, 1, p->gamma, p->dx, p->dy, max_steps, false));
    int rc = 0;
    for (int m = 0; m < max_steps && rc == 0; m++) {
        bool frame_done = false;
        // steps after the first: the ghost frames of both buffers, the minimum of the last stage's
        // CFL partials and the dt policy in ONE launch (k_fill_frame2_policy, round 6) -- they were
        // k_fill_x + k_fill_y inside the step, k_copy_frame4, k_min_one and k_dt_policy: five
        // launches, 30 us of a 0.64 ms step at 2048^2; the policy alone where the step has to fill
        rc = m == 0 ? rk_first_iteration(r, s, p, &frame_done) : evolve_between(r, m, true, false, &frame_done);
        if (rc) break;
        s->frame_prefilled = frame_done;
        rc = comp_rk_step_any(s, p, k, nstages, a, b, 0.0, s->d_scal, &r.dmin);
        r.take_pending();
        if (rc == 0) rc = evolve_particles(r);
    }
    s->frame_prefilled = false;
    PYRO_TRY(rc);
    rc = evolve_close(r, pol, steps_done, dts_out, true, false);
    s->cfl_is_global = false;
    return rc;
}

int pyrohip_comp_rk_evolve(pyrohip_state *y, const pyrohip_comp_params *p, pyrohip_state *k, int nstages,
                           const double *a, const double *b, double cfl, pyrohip_dt_policy *pol,
                           int max_steps, int *steps_done, double *dts_out)
{
    return pyrohip_comp_rk_evolve_p(y, p, k, nstages, a, b, cfl, pol, max_steps, steps_done, dts_out, nullptr,
                                    nullptr);
}

int pyrohip_comp_rk_rhs(pyrohip_state *y, const pyrohip_comp_params *p, pyrohip_state *k, int slot)
{
    PYRO_TRY(check_comp(y, p));
    PYRO_REQUIRE(k && k->ctx == y->ctx, "k state missing or on another context");
    PYRO_REQUIRE(k->g.nx == y->g.nx && k->g.ny == y->g.ny && k->g.ng == y->g.ng,
                 "k state must have the geometry of the stage state");
    PYRO_REQUIRE(slot >= 0 && 4 * (slot + 1) <= k->nvar, "slot outside the k state");
    PYRO_TRY(check_riemann(p, __func__));
    PYRO_TRY(check_sponge(p, __func__));
    if (p->well_balanced) {
        // reconstruction.py:24-25; no geometry terms in compressible_rk/fluxes.py anyway
        PYRO_REQUIRE(p->limiter == 1, "well_balanced only works for limiter == 1");
        PYRO_REQUIRE(!y->sph && y->nvar == 4, "well_balanced: a 4-variable state on a Cartesian grid");
    }
    // one launch of the row-marching kernel's method-of-lines instance where the call takes it
    // (takes_wave_kernel); the staged kernels otherwise (small grids, the sponge, the well-balanced
    // reconstruction)
    const bool wave = !p->do_sponge && !p->well_balanced && y->nvar == 4 && takes_wave_kernel(y->g, p);
    if (wave)
        return PYRO_BUILD(p->fast_math, comp_rk_rhs_wave(y, p, k, slot));
    return PYRO_BUILD(p->fast_math, comp_rk_rhs(y, p, k, slot));
}

// compressible_fv4 (csrc/comp_fv4.hip): the 4th-order right-hand side of a ghost-filled state
int pyrohip_comp_fv4_rhs(pyrohip_state *y, const pyrohip_comp_params *p, pyrohip_state *k, int slot)
{
    PYRO_TRY(check_comp(y, p));
    PYRO_REQUIRE(y->g.ng == 4, "compressible_fv4 needs ng = 4 (the reference's grid)");
    PYRO_TRY(check_not_well_balanced(p, __func__));
    PYRO_REQUIRE(!y->sph, "compressible_fv4 has no SphericalPolar geometry terms");
    PYRO_REQUIRE(k && k->ctx == y->ctx, "k state missing or on another context");
    PYRO_REQUIRE(k != y && k->d != y->d,
                 "k must not be the stage state: a tile would read cells that other tiles have "
                 "already overwritten");
    PYRO_REQUIRE(k->g.nx == y->g.nx && k->g.ny == y->g.ny && k->g.ng == y->g.ng,
                 "k state must have the geometry of the stage state");
    PYRO_REQUIRE(slot >= 0 && 4 * (slot + 1) <= k->nvar, "slot outside the k state");
    PYRO_TRY(check_sponge(p, __func__));
    return PYRO_BUILD(p->fast_math, comp_fv4_rhs(y, p, k, slot));
}

// fv.py:31-39 for variable `var` (-1: every variable, in order): fill its ghost cells, then
// a + dx^2 lap(a) / 24 on the interior
int pyrohip_state_from_centers(pyrohip_state *s, int var, double dx, double dy)
{
    PYRO_REQUIRE(s, "NULL state");
    PYRO_REQUIRE(var >= -1 && var < s->nvar, "variable index out of range");
    PYRO_REQUIRE(dx > 0 && dy > 0, "bad dx/dy");
    PYRO_REQUIRE(s->g.ng >= 1, "from_centers needs ghost cells");
    double *scratch = nullptr;
    PYRO_CHECK_HIP(hipMalloc((void **)&scratch, s->g.plane * sizeof(double)));
    int rc = 0;
    for (int n = (var < 0 ? 0 : var); n < (var < 0 ? s->nvar : var + 1) && rc == 0; n++) {
        rc = pyrohip_fill_bc(s, n);
        if (rc == 0) rc = exact::state_from_centers(s, n, dx, dy, scratch);
    }
    if (rc == 0) PYRO_CHECK_HIP(hipStreamSynchronize(s->ctx->stream));
    (void)hipFree(scratch);
    s->next_cfl_min = -1.0;
    s->ghost_by_rules = false;
    return rc;
}

// compressible_sdc/simulation.py:85-87: dst <- src + dt/2 (k_new - k_old) + dt/24 sum_q cq[q] k_q
int pyrohip_comp_sdc_update(pyrohip_state *dst, const pyrohip_state *src, const pyrohip_state *k,
                            int slot_new, int slot_old, const int *slots_q, const double *cq, double dt)
{
    PYRO_REQUIRE(dst && src && k && slots_q && cq, "NULL argument");
    PYRO_REQUIRE(dst->nvar == src->nvar && dst->g.plane == src->g.plane && dst->g.plane == k->g.plane &&
                     dst->g.nx == k->g.nx && dst->g.ny == k->g.ny,
                 "geometries differ");
    PYRO_REQUIRE(dst->ctx == src->ctx && dst->ctx == k->ctx, "states live on different contexts");
    const int nslots = k->nvar / dst->nvar;
    PYRO_REQUIRE(slot_new >= 0 && slot_new < nslots && slot_old >= 0 && slot_old < nslots,
                 "slot outside the k state");
    for (int q = 0; q < 3; q++) PYRO_REQUIRE(slots_q[q] >= 0 && slots_q[q] < nslots, "slot outside the k state");
    PYRO_TRY(exact::comp_sdc_update(dst, src, k, slot_new, slot_old, slots_q, cq, dt));
    dst->next_cfl_min = -1.0;
    dst->ghost_by_rules = false;
    return 0;
}

}  // extern "C"

// ---- compressible_fv4 / compressible_sdc: batches of steps on the device ----
// What both loops ask of the state that is stepped and of a state that stands beside it (stage state,
// node states, the k state); `fn` names the entry point in the messages.
static int check_fv4_run(pyrohip_state *y, const pyrohip_comp_params *p, const char *fn)
{
    PYRO_TRY(check_comp(y, p));
    PYRO_REQUIRE(y->g.ng == 4, "compressible_fv4 needs ng = 4 (the reference's grid)");
    PYRO_REQUIRE(!y->sph, "compressible_fv4 has no SphericalPolar geometry terms");
    PYRO_TRY(check_sponge(p, __func__));
    const char *why = nullptr;
    if (p->well_balanced) why = "compressible.well_balanced is not carried";
    else if (y->user_bc || y->ramp_bc) why = "hse / ambient / ramp sides are not carried";
    else if (y->nb_set || y->ctx->global_cfl) why = "a slab of a decomposed run is not carried";
    else if (y->ext_old) why = "a host-evaluated source is not carried";
    else if (!same_index_map_kinds(y, false)) why = "outflow / reflect / periodic sides only";
    else if (y->g.nx < y->g.ng || y->g.ny < y->g.ng) why = "fewer interior cells than ghost cells in a direction";
    if (why) {
        set_error(std::string(fn) + ": device-side stepping: " + why);
        return PYROHIP_ERR_ARG;
    }
    return 0;
}
static int check_fv4_beside(const pyrohip_state *y, const pyrohip_state *o, int planes, const char *what)
{
    PYRO_REQUIRE(o && o->ctx == y->ctx, std::string(what) + " missing or on another context");
    PYRO_REQUIRE(o != y && o->d != y->d,
                 std::string(what) + " must not be the state that is stepped: its cells are read while the "
                                     "other one's are written");
    PYRO_REQUIRE(o->g.nx == y->g.nx && o->g.ny == y->g.ny && o->g.ng == y->g.ng && o->nvar >= planes,
                 std::string(what) + " must have the geometry of the state and enough planes");
    return 0;
}
// the run both loops share: open, per iteration the policy and the solver's step, close.  step(S, part)
// enqueues one step that ends with fv4_final (new state and ghost frame in the other buffer, CFL
// partials in part); last_frame: the array whose ghost frame the state handed back carries -- nullptr:
// the other buffer's (the state before the last step), else that array's (the last SDC node)
template <class Step>
static int fv4_run(pyrohip_state *s, const pyrohip_comp_params *p, double cfl, pyrohip_dt_policy *pol,
                   int max_steps, int *steps_done, double *dts_out, const double *last_frame, Step step)
{
    pyrohip_ctx *c = s->ctx;
    PYRO_REQUIRE(pol && steps_done && max_steps >= 1, "NULL argument / max_steps must be positive");
    PYRO_TRY(state_alt(s));
    // (as much as comp_rk_cfl_min_device asks for: the buffer must not move while the run is enqueued)
    const int nparts = exact::fv4_final_parts(s->g);
    PYRO_TRY(c->reduce.ensure(((size_t)(nparts > 65536 ? nparts : 65536) + 2 * 8 * 128 + 256 + 2) *
                              sizeof(double)));    // (256: reduce.h's kMinStageBlocks)
    double *part = (double *)c->reduce.p;
    EvolveRun r;
    // the final update writes the ghost frame of the state it leaves and stores nothing on an inactive
    // iteration: the close neither rebuilds a frame nor fills the state after an invalid step
    r.own_frames = true;
    PYRO_TRY(evolve_open(r, s, pol, cfl, 1, p->gamma, p->dx, p->dy, max_steps, false));
    int rc = 0;
    for (int m = 0; m < max_steps && rc == 0; m++) {
        bool frame_done = false;
        rc = m == 0 ? rk_first_iteration(r, s, p, &frame_done) : evolve_between(r, m, false, false, &frame_done);
        if (rc) break;
        rc = step(r.d_scal, part);
        // the next policy call takes the minimum of the partials itself and keeps it in the step scalars
        // (min0), which the close reads back anyway
        r.pend = part;
        r.npend = nparts;
        r.dmin = &s->d_scal->min0;
        state_swap_alt(s);
    }
    PYRO_TRY(rc);
    rc = evolve_close(r, pol, steps_done, dts_out, false, false);
    s->cfl_is_global = false;
    if (rc == 0 && *steps_done >= 1)
        PYRO_TRY(exact::fv4_copy_frame(s, last_frame ? last_frame : s->alt_base + geom_lead(s->g)));
    // the minimum of the last launch belongs to the state only if that launch advanced it
    if (rc == 0 && *steps_done == max_steps) s->next_cfl_min = r.H.min0;
    return rc;
}

extern "C" {

// Up to max_steps steps of the compressible_fv4 driver loop (pyro_sim.py:241-281 with
// compressible_rk/simulation.py:46-104 and the right-hand side of compressible_fv4) under the run
// protocol of DESIGN.md 3.6.1.  stage / k: the states RKIntegrator.set_start makes.  particles: none is
// carried (refused).
int pyrohip_comp_fv4_evolve_p(pyrohip_state *y, const pyrohip_comp_params *p, pyrohip_state *stage,
                              pyrohip_state *k, int nstages, const double *a, const double *b, double cfl,
                              pyrohip_dt_policy *pol, int max_steps, int *steps_done, double *dts_out,
                              pyrohip_particles *particles, const pyrohip_particle_params *)
{
    PYRO_TRY(check_rk(y, p, k, nstages, a, b));
    PYRO_TRY(check_fv4_beside(y, k, 4 * nstages, "the k state"));
    PYRO_TRY(check_fv4_beside(y, stage, 4, "the stage state"));
    PYRO_REQUIRE(stage != k && stage->d != k->d, "k must not be the stage state");
    PYRO_REQUIRE(!particles, "device-side stepping: compressible_fv4 carries no tracer particles");
    PYRO_TRY(check_fv4_run(y, p, __func__));
    return fv4_run(y, p, cfl, pol, max_steps, steps_done, dts_out, nullptr,
                   [&](const StepScalars *S, double *part) -> int {
                       PYRO_TRY(PYRO_BUILD(p->fast_math, comp_fv4_rhs_run(y, p, k, 0, S, y->d_flag)));
                       for (int st = 1; st < nstages; st++) {
                           PYRO_TRY(exact::fv4_stage_start(stage, y, k, a + st * nstages, st, S));
                           PYRO_TRY(PYRO_BUILD(p->fast_math, comp_fv4_rhs_run(stage, p, k, st, S, y->d_flag)));
                       }
                       return exact::fv4_final(y, y, k, b, nstages, p, S, part);
                   });
}

int pyrohip_comp_fv4_evolve(pyrohip_state *y, const pyrohip_comp_params *p, pyrohip_state *stage,
                            pyrohip_state *k, int nstages, const double *a, const double *b, double cfl,
                            pyrohip_dt_policy *pol, int max_steps, int *steps_done, double *dts_out)
{
    return pyrohip_comp_fv4_evolve_p(y, p, stage, k, nstages, a, b, cfl, pol, max_steps, steps_done, dts_out,
                                     nullptr, nullptr);
}

// ... and of compressible_sdc (compressible_sdc/simulation.py:48-127): 9 right-hand sides and 8 node
// updates per step.  node1 / node2 / k (5 slots of 4 planes): compressible_sdc.Simulation._scratch.
int pyrohip_comp_sdc_evolve_p(pyrohip_state *y, const pyrohip_comp_params *p, pyrohip_state *node1,
                              pyrohip_state *node2, pyrohip_state *k, double cfl, pyrohip_dt_policy *pol,
                              int max_steps, int *steps_done, double *dts_out, pyrohip_particles *particles,
                              const pyrohip_particle_params *)
{
    PYRO_TRY(check_comp(y, p));
    PYRO_REQUIRE(y->g.ng == 4, "compressible_sdc needs ng = 4 (the reference's grid)");
    PYRO_TRY(check_fv4_beside(y, k, 4 * 5, "the k state"));
    PYRO_TRY(check_fv4_beside(y, node1, 4, "the state of node 1"));
    PYRO_TRY(check_fv4_beside(y, node2, 4, "the state of node 2"));
    PYRO_REQUIRE(node1 != node2 && node1->d != node2->d && node1->d != k->d && node2->d != k->d,
                 "the node states and the k state must be three different states");
    PYRO_REQUIRE(!particles, "device-side stepping: compressible_sdc carries no tracer particles");
    PYRO_TRY(check_fv4_run(y, p, __func__));
    // sdc_integral (simulation.py:20-36): dt/24 (c0 A_0 + c1 A_1 + c2 A_2) from node m to m + 1
    static const double C[2][3] = {{5.0, 8.0, -1.0}, {-1.0, 8.0, 5.0}};
    return fv4_run(y, p, cfl, pol, max_steps, steps_done, dts_out, (const double *)node2->d,
                   [&](const StepScalars *S, double *part) -> int {
                       pyrohip_state *U[3] = {y, node1, node2};
                       PYRO_TRY(PYRO_BUILD(p->fast_math, comp_fv4_rhs_run(y, p, k, 0, S, y->d_flag)));
                       int old[3] = {0, 0, 0};          // A_kold[m] -> slot
                       for (int it = 0; it < 4; it++) {
                           int nw[3] = {0, 0, 0}, next_free = 1;
                           for (int m = 0; m < 3; m++) {
                               if (m > 0) {
                                   while (next_free == old[1] || next_free == old[2]) next_free++;
                                   nw[m] = next_free++;
                                   PYRO_TRY(PYRO_BUILD(p->fast_math,
                                                       comp_fv4_rhs_run(U[m], p, k, nw[m], S, y->d_flag)));
                               }
                               if (m < 2)
                                   PYRO_TRY(exact::fv4_sdc_node(U[m + 1], U[m], k, nw[m], old[m], old, C[m], S,
                                                                y->d_flag));
                           }
                           old[1] = nw[1]; old[2] = nw[2];
                       }
                       // the new solution: the last node, floored by its right-hand side
                       return exact::fv4_final(y, node2, k, nullptr, 0, p, S, part);
                   });
}

int pyrohip_comp_sdc_evolve(pyrohip_state *y, const pyrohip_comp_params *p, pyrohip_state *node1,
                            pyrohip_state *node2, pyrohip_state *k, double cfl, pyrohip_dt_policy *pol,
                            int max_steps, int *steps_done, double *dts_out)
{
    return pyrohip_comp_sdc_evolve_p(y, p, node1, node2, k, cfl, pol, max_steps, steps_done, dts_out, nullptr,
                                     nullptr);
}

int pyrohip_comp_stage_dump(pyrohip_state *s, int stage_id, double *out)
{
    PYRO_REQUIRE(s && out, "NULL argument");
    return exact::comp_stage_dump(s, stage_id, out);
}

}  // extern "C"

// the tiles of the Runge-Kutta stage kernel on an nx x ny grid (comp_rk_tile.hip; no kernel runs):
// cells per tile along x and y, number of tiles -- tests place their shapes on the kernel's seams
extern "C" int pyrohip_comp_rk_tile_geometry(int nx, int ny, int *tx, int *ty, int *ntiles)
{
    PYRO_REQUIRE(tx && ty && ntiles, "NULL argument");
    PYRO_REQUIRE(nx >= 1 && ny >= 1, "nx, ny must be positive");
    pyro::exact::rk_tile_geometry(nx, ny, tx, ty, ntiles);
    return 0;
}

extern "C" int pyrohip_sph_wave_geometry(int nx, int ny, int ng, int num_cus, int march_rows, int *out7)
{
    PYRO_REQUIRE(out7 && nx > 0 && ny > 0 && ng >= 0 && march_rows >= 0, "bad argument");
    return pyro::exact::sph_wave_geometry(nx, ny, ng, num_cus, march_rows, out7);
}

extern "C" int pyrohip_comp_wave_geometry(int nx, int ny, int ng, int num_cus, int march_rows, int *out6)
{
    PYRO_REQUIRE(out6 && nx > 0 && ny > 0 && ng >= 0, "bad argument");
    return pyro::exact::comp_wave_geometry(nx, ny, ng, num_cus, march_rows, out6);
}

extern "C" int pyrohip_comp_wave_plan(int nx, int ny, int ng, int num_cus, int march_rows, int neighbours, int *out11)
{
    PYRO_REQUIRE(out11 && nx > 0 && ny > 0 && ng >= 0 && march_rows >= 0, "bad argument");
    return pyro::exact::comp_wave_plan(nx, ny, ng, num_cus, march_rows, neighbours, out11);
}
