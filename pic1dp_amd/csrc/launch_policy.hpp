// launch_policy.hpp -- the launch shape of every marker kernel as a pure function of the device's size, the grid, the
// marker count and three knobs.  No context, no HIP call: capi_step.cpp fills LaunchPolicy from the context and launches
// what comes back; tests/test_launch_policy_host.py pins every shape on the host (include/pic1dp_probe.h).  The
// diagnostics passes of output_all have theirs here too (diag_launch; tests/test_diag_launch_host.py).
// The functions return a shape whose LDS exceeds PARTICLE_LDS_CAP as it is: the callers decide what to run instead.
#pragma once
#include "kernels.hpp"

namespace pic1dp {

constexpr size_t kCuLds = 160 * 1024, kStaticLds = 1024;  // LDS of a CU; static LDS of a marker kernel (the exp table)

// what the policy needs from the context
struct LaunchPolicy {
  int num_cu;       // compute units of the device
  int threads_req;  // pic1dp_hip_set_launch: threads per workgroup asked for by hand (0: the measured choice)
  int bpc_req;      // ... and workgroups per CU (0: the measured choice)
  int osub_req;     // PIC1DP_OSUB: grid size in units of the resident one (0: auto)
};

// a one-pass launch and the workgroups that fill the CUs (the grid is that, or a multiple: oversubscription)
struct PredLaunch {
  LaunchCfg lc;
  int64_t resident;
};

// sub-step kernels (k_push, k_push<FUSED>, k_deposit): E tile and / or rho tile
// exact: the rho tile of kind 1 of the charge sum (two words per cell)
LaunchCfg particle_launch(const LaunchPolicy &p, int nx, int64_t np, bool with_E, bool with_rho, bool exact = false);
// whole-step kernels k_step_half (full = false) and k_step_full
LaunchCfg step_launch(const LaunchPolicy &p, int nx, int64_t np, bool full, bool exact);
// k_step_full<DIAG>: one workgroup of 1024 threads per CU, grid tiles + the histograms of nx_opd x nv_opd cells in its LDS
LaunchCfg step_diag_launch(const LaunchPolicy &p, int nx, int64_t np, bool exact, int nx_opd, int nv_opd);
// the one-pass kernels: k_step_one (pred_kind 1, nmode kept modes), k_step_sums (pred_kind 2; exp_bearing: the
// distribution's -f0'/f0 bears an exp) and k_step_one<PRIV> (priv)
PredLaunch pred_launch(const LaunchPolicy &p, int nx, int nmode, int64_t np, bool priv, int pred_kind, bool exp_bearing);
// may the prologue of this one-pass launch solve the previous step's field (kernels.hpp FusedSolve)?  It needs a first and
// a last wave of its own (lean_forward_sums runs its chains in wave 0 while the last wave adds up the copies of the six
// sums), and a grid within the resident one: EVERY workgroup runs the solve, an oversubscribed grid pays it per round
inline bool fits_fused_solve(const PredLaunch &pl) {
  return pl.lc.blocks <= pl.resident && pl.lc.threads >= 128 && pl.lc.threads % 64 == 0;
}

// ---- the share of the marker state a non-temporal one-pass launch keeps in the Infinity Cache ----
// The 64-pair chunks at the HEAD of this species' slab that k_step_one / k_step_sums access with plain loads and stores
// (StepArgsDev::plain_chunks) while the rest streams non-temporally: non-temporal accesses pass the cache by, so the plain
// share stays resident from step to step.  All species together get kPlainStateBytes of state (x, v, w, p: 32 B a marker,
// 4096 B a chunk), each species its share by marker count.  Measured on the pure 4-read / 3-write stream
// (tools/sweep_direction_probe.py, profiles/r23/sweep_probe.log) at 1e7, 1.25e7 and 1e8 markers: 224 ... 272 MiB at the
// head do alike (as 2 x 112 ... 2 x 128 MiB at the two ends do), less keeps less, more begins to thrash.
// 0: a plain launch (the state fits the cache as it is), no markers.
constexpr int64_t kPlainStateBytes = static_cast<int64_t>(256) << 20;
int64_t stream_plain_chunks(int64_t np_all_species, int64_t np_species, bool nt);

// ---- the diagnostics passes of output_all (kernels_diag.hip) ----
constexpr size_t kDiagLdsCap = 150 * 1024;  // a workgroup's LDS copy of the histograms: one workgroup of 1024 threads per CU
constexpr int kEnergyBlocks = 1024;         // most workgroups a pass over tail slots gets
// kind 0: k_ptcldist, the workgroup's copy [3 nxo nvo + 3 nvo] doubles + block_sum scratch and the drawn chunks' counter;
// kind 1: k_ptcldist_exact, one 64-bit word per bin and plane + the kinetic words and the counter
DiagLaunch diag_launch(int kind, int64_t np, int nxo, int nvo, int num_cu);
// workgroups of 256 threads for the kinetic sums of ntail tail slots (0: none)
int tail_sum_blocks(int64_t ntail);

// ---- the velocity moments on the field grid (kernels_moments.hip; include/pic1dp_hip.h pic1dp_hip_moments) ----
// The passes of one call: which = 1 (p), 2 (w), 3 (both, p first) selects 4 or 8 planes in output order (weight set, then
// power of v).  A pass holds at most kDiagLdsCap / (8 nx) of them in its workgroup's LDS, as doubles [plane][cell]; groups
// are cut in output order, never across two weight sets unless all eight fit, and only as the kernel is instantiated:
// eight planes (nx <= 2400), four (nx <= 4800: one pass per weight set) or two (powers {0, 1}, then {2, 3}).  Every nx a
// context accepts (<= 8192) is served from LDS.  One workgroup of 1024 threads per CU, never more than the marker pairs ask
// for; non-temporal loads once the arrays the pass reads (x, v and p and / or w: 24 or 32 B per marker) exceed the
// threshold of diag_launch.  npass = 0: an unknown `which`, w asked of a full-f run (deltaf = 0), or nx out of range.
MomentsPlan moments_plan(int nx, int which, int deltaf, int64_t np, int num_cu);
// The passes of pic1dp_hip_moments_exact (k_moments_exact): groups, bytes (one 64-bit word per plane and cell), NT, weight
// sets, powers and first planes are moments_plan's; the grid is max(1, min(num_cu, ceil(np / 2^17))) workgroups, the exact
// diagnostics' rule: every workgroup flushes two global atomics per non-zero word at its end, which costs what a few trips cost.
MomentsPlan moments_plan_exact(int nx, int which, int deltaf, int64_t np, int num_cu);

// ---- the wave-particle power on the output grid (kernels_power.hip; include/pic1dp_hip.h pic1dp_hip_power) ----
// The passes of one call: which = 1 (p), 2 (w), 3 (both, p first) selects one or two planes of nx_opd x nv_opd doubles.  A
// workgroup's dynamic LDS begins with the E tile, tile = round16(8 (nx + 1)) bytes (cell nx: the push's guard), the planes
// follow it; with plane = 8 nx_opd nv_opd and cap = kDiagLdsCap:
//   tile + nsets plane <= cap : one pass, all sets, planes in LDS
//   tile + plane <= cap       : one pass per set, in output order, planes in LDS
//   else                      : one pass, all sets, planes straight in memory (dynamic LDS: the tile alone)
// One workgroup of 1024 threads per CU, never more than the marker pairs fill; non-temporal loads once the arrays a pass
// reads (x, v and p and / or w: 24 or 32 B per marker) exceed the threshold of diag_launch.  npass = 0: an unknown `which`,
// w asked of a full-f run (deltaf = 0), nx < 1, nx_opd < 1, nv_opd < 2, or a tile beyond the cap (no context has such a grid).
constexpr size_t power_tile_bytes(int nx) { return (sizeof(double) * (static_cast<size_t>(nx) + 1) + 15) & ~static_cast<size_t>(15); }
PowerPlan power_plan(int nx, int nx_opd, int nv_opd, int which, int deltaf, int64_t np, int num_cu);
// The passes of pic1dp_hip_power_exact (k_power_exact): passes, bytes (the tile, and one 64-bit word per set and bin), NT,
// weight sets and first sets are power_plan's; the grid is max(1, min(num_cu, ceil(np / 2^17))) workgroups, the rule of
// the exact diagnostics and the exact moments.
PowerPlan power_plan_exact(int nx, int nx_opd, int nv_opd, int which, int deltaf, int64_t np, int num_cu);

// ---- select and gather markers (kernels_select.hip; include/pic1dp_hip.h pic1dp_hip_select) ----
// The count pass and the write pass of a selection over np valid markers, one shape for both: chunks of SELECT_CHUNK_PAIRS
// pairs (kernels.hpp), nchunk = max(1, ceil((np / 2) / chunk pairs)) for np > 0 (one marker alone is the odd last marker of
// chunk 0) and 0 for np = 0; workgroups of ONE wave (64 threads), 24 per CU = six waves per SIMD, what 79 registers and 106
// scalar ones admit, never more than there are chunks,
// at least one.  A wave of its own needs nobody's totals: the write pass's barrier per trip is free, where at 512 threads x 3
// it costs a fifth of the selection (measured at 1e8 markers, DESIGN.md 2.18: 0.674 against 0.803 ms; 1024 x 2: 1.07 ms).
// pic1dp_hip_set_launch's threads and workgroups per CU are taken literally when given
// (threads_req a multiple of 64, <= 1024; 0: the choice above): the result does not depend on them.  Non-temporal loads
// once x and v (16 B per marker) exceed the threshold of diag_launch.  The prefix sum runs in one workgroup of 1024.
SelectPlan select_plan(int64_t np, int num_cu, int threads_req, int bpc_req);

// ---- the exact phase-space histogram on a caller's window and grid (kernels_zoom.hip; include/pic1dp_hip.h pic1dp_hip_zoom) ----
// The passes of one call: which (bit 0 markr, 1 total, 2 pertb) selects n planes of nvb rows of nxb cells, one signed 64-bit
// word per (plane, cell) in a workgroup's LDS, kDiagLdsCap / 8 = 19 200 words at most.  Every pass holds ALL selected planes
// of a band of whole v rows: a row of all three is at most 3 x 4096 = 12 288 words, so it always fits, and a pass per group
// of planes would sweep x and v once more for the same rows.  With R = 19 200 / (n nxb) rows a pass:
//   nvb <= R                        : one pass, every row (LDS)
//   ceil(nvb / R) <= kZoomPassCap   : that many band passes, R rows each, the last the remainder (LDS)
//   else                            : one pass, the terms straight into the global (hi, lo) rows (bytes 0)
// pass_cap: kZoomPassCap, the measured crossover -- at 1e8 markers four band passes take 2.31 ms, the pass into memory 2.6 ms
// whatever the grid, eight band passes 4.34 ms; a measurement varies it (tools/zoom_bench.py).
// One workgroup of 1024 threads per CU, the exact kinds' grid max(1, min(num_cu, ceil(np / 2^17))); non-temporal loads once
// the arrays a pass reads (x, v and p and / or w) exceed the threshold of diag_launch.  npass = 0: which outside 1..7, pertb
// asked of a full-f run (deltaf = 0), nxb or nvb outside 1..4096, more than 2^20 cells.
constexpr int kZoomPassCap = 4;
ZoomPlan zoom_plan(int nxb, int nvb, int which, int deltaf, int64_t np, int num_cu, int pass_cap = kZoomPassCap);

// ---- the Fourier-Hermite spectrum (kernels_hermite.hip; include/pic1dp_hip.h pic1dp_hip_hermite) ----
// One pass whatever is asked: workgroups of 256 threads, every wave with its two LDS tiles (HERM_WAVE_LDS: 66 KiB a
// workgroup, two a CU) and nb = 4 (nherm <= 64), 8 (<= 128) or 16 blocks of sixteen Hermite rows in its accumulator registers.
// The grid: two workgroups per CU, but a workgroup sweeps at least kHermiteMinTrips chunks of 64 markers per wave before
// another one is started (its flush is up to 16 nherm global atomics); at least one.  Non-temporal loads once the arrays
// the pass reads (x, v and p and / or w: 24 or 32 B per marker) exceed the threshold of diag_launch.  partials: what is
// merged into one output word, blocks * (waves + 1) -- every wave's accumulator into its workgroup's LDS word, every
// workgroup's word into memory.  blocks = 0: an unknown `which`, w asked of a full-f run (deltaf = 0), nherm outside
// 1..256, nmodes < 1 or more than sixteen columns.
constexpr int kHermiteMinTrips = 16;
HermitePlan hermite_plan(int nherm, int nmodes, int which, int deltaf, int64_t np, int num_cu);

// ---- the state digest (kernels_digest.hip) ----
// one streaming pass over the nalloc slots of a species, marker pairs as double2: workgroups of 256 threads, eight per CU
// (no LDS to speak of, few registers: the CUs fill with waves whose loads cover the latency), never more than the pairs
// ask for; non-temporal loads above the threshold of diag_launch
DigestLaunch digest_launch(int64_t nalloc, int num_cu);

// ---- the on-device particle load (kernels_load.hip) ----
// one streaming pass that writes the nalloc slots of a species: workgroups of 256 threads that take whole chunks of
// LOAD_CHUNK markers (a tile group: 128 KiB of the slab in one piece), eight per CU, never more than there are chunks, at
// least one; non-temporal stores once the bytes written exceed the threshold of diag_launch
LoadLaunch load_launch(int64_t nalloc, int num_cu);

}  // namespace pic1dp
