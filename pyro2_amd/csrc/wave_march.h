// What the row-marching kernels share: one wavefront marches a strip of rows, its
// column neighbours sit in the neighbouring lanes, and the strips are dealt to the resident wavefront
// slots -- k_ctu_wave (comp_wave.hip), k_sph_wave (comp_sph_wave.hip), k_sw_wave (swe.hip),
// k_adv_step / k_adv_multi (advection.hip), the marching and band smoothers (mg_march.hip,
// multigrid.hip).  Included at file scope (never inside namespace pyro::PYRO_NS).
#pragma once
#include <hip/hip_runtime.h>

// stage boundary: the scheduler may not move instructions across it.  The stages of a row are
// written in the order that keeps the live ranges short (a value is produced right before the
// Riemann problem that consumes it); left alone, the scheduler interleaves the stages for ILP and
// pushes the kernel over 256 VGPRs.
#if defined(PYRO_EMU)
#define PYRO_SCHED_FENCE() do {} while (0)
#else
#define PYRO_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif

namespace pyro {

// ---- lane moves ----
// value of the same variable in lane l-1 / l+1.  The ends of the wavefront are
// apron lanes whose results are never stored, but what they compute matters
// for speed: a wavefront executes every lazily evaluated branch (flattening,
// the shock branches of the wave-speed estimate) that ANY lane takes.  The DPP
// moves therefore ROTATE (lane 0 reads lane 63: a finite physical state, equal
// to its own in uniform regions) -- with shifts + bound_ctrl the end lanes read
// 0, went to NaN and dragged the wavefront through the slow paths (+8 v_rsq /
// v_rcp per row, PMC); shifts that keep the own value need a register copy in
// front of every move (the `old` operand is tied to the destination).  The
// shuffle variant (the emulator's) keeps the own value.  gfx950 keeps the GFX9
// whole-wave DPP shifts (wave_shr:1 / wave_shl:1 move data across all 64 lanes,
// tools/dpp_probe.hip): two
// v_mov_b32_dpp per double, a register-to-register VALU move without the
// LDS-crossbar round trip of ds_bpermute (__shfl_up / __shfl_down).
#if !defined(PYRO_EMU)
template <int CTRL> __device__ __forceinline__ double lane_dpp(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, true);
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_from_lower(double v) { return lane_dpp<0x13C>(v); }   // wave_ror:1
__device__ __forceinline__ double lane_from_upper(double v) { return lane_dpp<0x134>(v); }   // wave_rol:1
#else
__device__ __forceinline__ double lane_from_lower(double v) { return __shfl_up(v, 1, 64); }
__device__ __forceinline__ double lane_from_upper(double v) { return __shfl_down(v, 1, 64); }
#endif

// ---- the priority of the two wavefronts of a SIMD ----
// The two wavefronts of a SIMD are arbitrated by age: the older one runs almost as if it
// were alone, the younger one gets what is left, and when the older one is done the younger
// finishes alone at half the issue rate -- measured per wavefront at 4096^2 (one round of
// resident wavefronts; tools/timeline_report.py): 1.11 M cycles for one half of the
// wavefronts, 1.56 M for the other half, on every SIMD.  With many rounds a new wavefront
// takes the place of the finished one and nothing is lost; with one or two rounds the
// tail is a third of the launch.  So the two take turns at the higher priority, a few
// rows each (by the wavefront's slot number on its SIMD), and finish together.
// Round 6, second half: the turns by phase are blind -- each wavefront counts its OWN rows, the two
// drift apart and the better duty changes with the strip length (tools/wave_timeline.py, 4096^2: the
// second wavefront ends 90 us before the first with seven eighths, 80 us after it with four, together with
// five; 3072^2 wants seven).  With a board (one word per SIMD and slot in device memory: common.h
// prio_board_acquire; the two wavefronts of a SIMD sit on one XCD = one L2) each tells the other how many
// rows it has left, a row late, and the one with more rows left takes the priority: the pair ends together
// whatever the strips.
// A kernel calls wave_prio_begin in front of its row loop, wave_prio_turn at the top of every iteration and
// wave_prio_publish right BEHIND the request of the next row.  The board's null test, the rows left and the phase
// are evaluated in here, inside the branch that uses them: evaluated at the call they changed the spill code of
// k_sph_wave (docs/HISTORY.md).  k_ctu_wave has its own copy of this code (comp_wave.hip says why): a fix goes
// to both.  GPU only: the emulator's variants do nothing.
#if !defined(PYRO_EMU)
struct WavePrio {
    int wslot;             // the wavefront's slot number on its SIMD
    bool board;            // the pair tells each other its rows left (otherwise: turns by phase and duty)
    int *mine, *other;     // ... the pair's two words on the board
    int tag, seen;         // ... the launch's tag; the other one's word, asked for an iteration ago
};
// uses_board: this instance of the kernel has the board protocol (it still takes the turns by phase where the
// launch brought no board)
__device__ __forceinline__ WavePrio wave_prio_begin(int *board, int tag, bool uses_board)
{
    unsigned hw_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
    WavePrio w{(int)(hw_id & 1u), uses_board && board != nullptr, nullptr, nullptr, tag, 0};
    if (w.board) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        int *const pair = board + 2 * (int)(((xcc & 15u) << 12) | ((hw_id >> 4) & 0xfffu));   // (SIMD, CU, SH, SE)
        w.mine = pair + w.wslot;
        w.other = pair + (w.wslot ^ 1);
    }
    return w;
}
// (the word goes out and the other one is asked for BEHIND the request of the next row: loads return in
// order, in front of it a miss of this word would hold up the row; workgroup scope -- sc0: through the
// CU's cache to the XCD's L2, the two wavefronts share both)
__device__ __forceinline__ void wave_prio_publish(WavePrio &w, int left)
{
    if (!w.board) return;
    __hip_atomic_store(w.mine, (w.tag << 16) | left, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    w.seen = __hip_atomic_load(w.other, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// iteration k of a strip whose first row is i0 and whose last iteration is `last`: last - k rows left (what the
// wavefront publishes); without a board the turns go by phase, two rows each, and duty (eighths of the time
// the second wavefront of the SIMD holds the priority, 0: age decides)
__device__ __forceinline__ void wave_prio_turn(const WavePrio &w, int k, int i0, int last, int duty)
{
    if (w.board) {
        // (the word asked for an iteration ago: complete with the row that arrived since)
        const int seen = __builtin_amdgcn_readfirstlane(w.seen);
        const int left = last - k;
        const int other_left = ((seen >> 16) == w.tag) ? (seen & 0xffff) : left;
        if (left > other_left) __builtin_amdgcn_s_setprio(1);
        else if (left < other_left) __builtin_amdgcn_s_setprio(0);
    } else if (duty > 0) {
        const int phase = ((k - i0) >> 1) & 7;
        if (w.wslot ? (phase < duty) : (phase >= duty)) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
    }
}
#else
struct WavePrio {};
__device__ __forceinline__ WavePrio wave_prio_begin(int *, int, bool) { return WavePrio{}; }
__device__ __forceinline__ void wave_prio_publish(WavePrio &, int) {}
__device__ __forceinline__ void wave_prio_turn(const WavePrio &, int, int, int, int) {}
#endif

// ---- strips ----
// one-round launches: as many strips as wavefront slots -- the first n_extra of the ncb column strips are cut into
// nsb + 1 row strips of equal length instead of nsb (a SIMD left with ONE wavefront gets little out of it and
// the launch lasts as long as its last wavefront: tools/wave_timeline.py)
inline int wave_fill_extra(int ncb, int nsb, int nx, int slots)
{
    const int nreg = ncb * nsb;
    if (nsb < 2 || nreg >= slots || nx / (nsb + 1) < 8) return 0;
    return slots - nreg < ncb ? slots - nreg : ncb;
}
// ... the kernel's half: strip sb of such a column strip is the rows [wave_extra_row(sb), wave_extra_row(sb + 1)) --
// nsb + 1 strips of equal length (to a row)
__device__ __forceinline__ int wave_extra_row(int sb, int nsb, int nx, int ilo)
{
    return ilo + (int)((long)sb * nx / (nsb + 1));
}
// row strips of L rows over nx rows: a last strip shorter than `join` rows joins its predecessor (join = the
// ghost width: the boundary strips of a slab must hold the ng rows the neighbour receives as its halo)
inline int wave_strip_count(int nx, int L, int join)
{
    int nsb = (nx + L - 1) / L;
    if (nsb > 1 && nx - (nsb - 1) * L < join) nsb--;
    return nsb;
}
// Rows per strip (a strip costs L + 8 iterations, of which the 8 warm-up ones are cheap: ~3 % of
// the instructions at L = 69).  What matters is the LAST round of resident wavefronts: the
// launch lasts ceil(wavefronts / slots) strip times, and a last round that fills a third to a
// half of the slots is the worst case -- measured at 8192^2 (147 column strips, 2048 slots,
// profiles/r04_march_sweep.txt): 59 rows = 9.98 rounds 2.525 ms, 74 rows = 7.97 rounds 2.525,
// 75 rows = 7.9 rounds 2.549, 64 rows = 9.19 rounds 2.576, 82 rows = 7.18 rounds 2.588, 69 rows =
// 8.54 rounds 2.624 (round 3's choice, by (rounds + 1/2)(L + 8) with fractional rounds), 112 rows
// = 5.31 rounds 2.628, 128 rows 2.688.  So: the strip length in lmin .. 160 rows that minimises
// (ceil(wavefronts / slots) + 1) x (L + 8) -- WHOLE rounds, plus a strip time for the stragglers of
// the last one (few long rounds end worse than many short ones: the two wavefronts of a SIMD are
// served oldest first) --, the shorter strip winning a tie.  One round when everything is resident at once
// (4096^2: 74 x 27 strips of 152 rows).
inline int wave_strip_rows(int nx, int ncb, int slots, int lmin)
{
    if (nx <= 32) return nx;
    long best_cost = -1;
    int best = 32;
    for (int L = lmin; L <= 160 && L <= nx; L++) {
        const int nsb = wave_strip_count(nx, L, 4);         // short last strip joins its predecessor
        const int Leff = (nx + nsb - 1) / nsb;                // longest strip
        const long waves = (long)ncb * nsb;
        const long rounds = (waves + slots - 1) / slots;
        // strip times: one round when everything is resident at once, otherwise whole rounds
        // + one more for the stragglers of the last one
        const long cost = (waves <= slots ? 1 : rounds + 1) * (Leff + 8);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = L; }
    }
    return best;
}

}  // namespace pyro
