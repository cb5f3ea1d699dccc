// launch_policy.cpp -- launch shapes of the marker kernels and of the diagnostics passes (launch_policy.hpp): arithmetic only
#include "launch_policy.hpp"

#include <algorithm>
#include <cmath>

namespace pic1dp {

namespace {

enum class Osub {
  Never,    // the resident grid
  IfAsked,  // a multiple of it only where PIC1DP_OSUB insists
  Auto,     // ... or where the markers per workgroup allow it
};

// Grid of a marker kernel: `resident` workgroups fill the CUs; with a grid of exactly that size the kernel ends
// when its slowest workgroup does, and the CUs do not all stream at the same rate.  A grid of several times that
// size lets the CUs that finish early take more of the work (tools/ab_one_shapes.sh: k_step_one at 1e8 markers
// 1.290 -> 1.238 ms with four times the resident workgroups) -- as long as a workgroup's share of the markers
// dwarfs what it pays once (staging and flushing tiles of nx cells): about 48 markers per cell, at most x4.
// Only where two workgroups share a CU (while one stages or flushes the other streams; alone on its CU a
// workgroup's turn-over idles it: k_step_sums at nx 4096, 0.935 -> 1.004 ms with twice the grid), and not for
// k_step_full, which measures 1-3 % slower that way (k_step_half 5 % faster; tools/ab_osub.sh).
// PIC1DP_OSUB=n insists on a factor (1: the resident grid).
int64_t oversubscribed(const LaunchPolicy &p, int nx, int64_t np, int64_t resident, Osub how) {
  if (how == Osub::Never) return resident;
  if (p.bpc_req > 0) return resident;  // a launch shape asked for by hand is taken literally
  int64_t f = p.osub_req;
  if (f <= 0 && how != Osub::Auto) return resident;
  if (f <= 0) {
    const int64_t per_wg = static_cast<int64_t>(48) * nx;
    f = (np / per_wg + resident / 2) / std::max<int64_t>(resident, 1);
  }
  f = std::max<int64_t>(1, std::min<int64_t>(f, p.osub_req > 0 ? 64 : 4));
  return resident * f;
}

// the tail of every shape: bpc workgroups on each CU are resident, the grid is that or a multiple of it, at most one
// workgroup per `threads` marker pairs, at least one
struct Grid {
  int64_t resident;
  int blocks;
};
Grid grid_of(const LaunchPolicy &p, int nx, int64_t np, int threads, int bpc, Osub how) {
  const int64_t resident = static_cast<int64_t>(p.num_cu) * bpc;
  const int64_t need = ((np >> 1) + threads - 1) / threads;
  const int64_t blocks = std::max<int64_t>(1, std::min(oversubscribed(p, nx, np, resident, how), need));
  return Grid{resident, static_cast<int>(blocks)};
}

// workgroups per CU of the sub-step and whole-step kernels: what the thread count suggests, what the LDS holds, what was
// asked for by hand (within what the LDS holds)
int workgroups_per_cu(const LaunchPolicy &p, int bpc, int by_lds) {
  if (bpc > by_lds) bpc = by_lds;
  if (p.bpc_req > 0) bpc = p.bpc_req < by_lds ? p.bpc_req : by_lds;
  return bpc < 1 ? 1 : bpc;
}

}  // namespace

LaunchCfg particle_launch(const LaunchPolicy &p, int nx, int64_t np, bool with_E, bool with_rho, bool exact) {
  LaunchCfg lc{};
  lc.lds = sizeof(double) * ((with_E ? static_cast<size_t>((nx + 2) & ~1) : 0) +
                             (with_rho ? (exact ? 2 : 1) * (static_cast<size_t>(nx) + 1) : 0));  // + guard cell
  int by_lds = lc.lds ? static_cast<int>(kCuLds / (lc.lds + kStaticLds)) : 8;
  if (by_lds < 1) by_lds = 1;
  int threads = p.threads_req > 0 ? p.threads_req : 512;
  if (p.threads_req <= 0 && by_lds * threads < 2048) threads = 1024;
  const int bpc = workgroups_per_cu(p, 2048 / threads, by_lds);
  lc.threads = threads;
  lc.blocks = grid_of(p, nx, np, threads, bpc, Osub::Never).blocks;
  return lc;
}

LaunchCfg step_launch(const LaunchPolicy &p, int nx, int64_t np, bool full, bool exact) {
  LaunchCfg lc{};
  lc.lds = step_lds_bytes(nx, full, exact);
  int by_lds = static_cast<int>(kCuLds / (lc.lds + kStaticLds));
  if (by_lds < 1) by_lds = 1;
  // two workgroups of 768 threads per CU (24 waves): measured inside one process
  // (tools/ab_launch.py) best or within 1 % of best from 6.4e6 to 1e8 markers --
  // fewer workgroups mean fewer LDS stagings and half as many global flush atomics
  // as four workgroups of 512, which cost k_step_half 25 % at 6.4e6 and 15 % at 2e7
  int threads = p.threads_req > 0 ? p.threads_req : 768;
  if (p.threads_req <= 0 && by_lds < 2) threads = 1024;
  const int bpc = workgroups_per_cu(p, p.threads_req > 0 ? 2048 / threads : (threads == 768 ? 2 : 1), by_lds);
  lc.threads = threads;
  lc.blocks = grid_of(p, nx, np, threads, bpc, !full && bpc >= 2 ? Osub::Auto : Osub::IfAsked).blocks;  // (not for k_step_full)
  return lc;
}

LaunchCfg step_diag_launch(const LaunchPolicy &p, int nx, int64_t np, bool exact, int nx_opd, int nv_opd) {
  LaunchCfg lc{};
  lc.lds = step_lds_bytes(nx, true, exact) + step_diag_lds_bytes(nx, nx_opd, nv_opd);
  lc.threads = 1024;
  lc.blocks = grid_of(p, nx, np, lc.threads, 1, Osub::Never).blocks;
  return lc;
}

PredLaunch pred_launch(const LaunchPolicy &p, int nx, int nmode, int64_t np, bool priv, int pred_kind, bool exp_bearing) {
  LaunchCfg lc{};
  lc.lds = priv ? step_one_private_lds_bytes(nx) : (pred_kind == 2 ? step_sums_lds_bytes(nx) : step_one_lds_bytes(nx, nmode));
  bool two = 2 * (lc.lds + kStaticLds) <= kCuLds;  // both workgroups resident: each also holds the static exp table
  int th2 = 768;
  int th1 = 1024;
  if (priv) {  // the private sums' slot stride is a compile-time constant: exactly that many threads
    th2 = th1 = STEP_PRIVATE_THREADS;
    if (STEP_PRIVATE_THREADS > 768) two = false;
  }
  if (pred_kind == 2 && !priv) {
    // k_step_sums keeps its registers: four waves per SIMD with the exp-bearing distributions (one
    // workgroup of 1024 per CU), eight with the others, which saturate the memory system with far fewer
    // (tools/ab_sums_shapes.sh: 1e8 markers, Maxwellian, nx 4096: 512 x 1 0.925 ms, 1024 x 1 0.965 ms)
    if (exp_bearing)
      two = false;
    else
      th1 = 512;
  }
  lc.threads = p.threads_req > 0 ? p.threads_req : (two ? th2 : th1);
  const int bpc = p.bpc_req > 0 ? p.bpc_req : (two ? 2 : 1);
  const Grid g = grid_of(p, nx, np, lc.threads, bpc, bpc >= 2 ? Osub::Auto : Osub::IfAsked);
  lc.blocks = g.blocks;
  return PredLaunch{lc, g.resident};
}

DiagLaunch diag_launch(int kind, int64_t np, int nxo, int nvo, int num_cu) {
  const size_t nxv = static_cast<size_t>(nxo) * nvo;
  DiagLaunch d{};
  d.threads = 1024;
  // x, v, p, w against the 256 MiB Infinity Cache: beyond it the pass streams
  d.nt = 32.0 * static_cast<double>(np) > 288.0 * 1048576.0;
  int64_t blocks;
  if (kind == 1) {
    d.lds = sizeof(long long) * (3 * nxv + 8) <= kDiagLdsCap;
    d.bytes = sizeof(long long) * ((d.lds ? 3 * nxv : 0) + 8);
    // A workgroup's flush costs what a few trips cost (two global atomics per non-zero bin), so a workgroup gets at least
    // 2^17 markers (64 trips) before a second one is started; never more workgroups than CUs (one copy per CU fits).
    blocks = std::min<int64_t>(np >> 17, num_cu);
  } else {
    const size_t hist = sizeof(double) * (3 * nxv + 3 * static_cast<size_t>(nvo));
    d.lds = hist <= kDiagLdsCap;
    d.bytes = (d.lds ? hist : 0) + 18 * sizeof(double);
    blocks = std::min<int64_t>(d.lds ? num_cu : static_cast<int64_t>(num_cu) * 2, ((np >> 1) + 1023) / 1024);
  }
  d.blocks = static_cast<int>(std::max<int64_t>(blocks, 1));
  return d;
}

MomentsPlan moments_plan(int nx, int which, int deltaf, int64_t np, int num_cu) {
  MomentsPlan m{};
  if (which < 1 || which > 3 || ((which & 2) && !deltaf) || nx < 1) return m;
  m.selected = which == 3 ? 8 : 4;
  const size_t fit = kDiagLdsCap / (sizeof(double) * static_cast<size_t>(nx));
  m.group = fit >= 8 && m.selected == 8 ? 8 : (fit >= 4 ? 4 : (fit >= 2 ? 2 : 0));
  if (m.group == 0) return m;   // (nx > 9600: no context has such a grid)
  m.npass = m.selected / m.group;
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(num_cu, ((np >> 1) + 1023) / 1024));
  for (int i = 0; i < m.npass; ++i) {
    MomentsPass &ps = m.pass[i];
    ps.first_plane = i * m.group;
    ps.planes = m.group;
    const int set = ps.first_plane / 4;          // of the sets selected, in output order
    ps.p = m.group == 8 || (which != 2 && set == 0);
    ps.w = m.group == 8 || which == 2 || set == 1;
    ps.kmask = m.group >= 4 ? 0xF : (ps.first_plane % 4 == 0 ? 0x3 : 0xC);
    ps.threads = 1024;
    ps.blocks = static_cast<int>(blocks);
    ps.bytes = sizeof(double) * static_cast<size_t>(m.group) * static_cast<size_t>(nx);
    ps.nt = 8.0 * (2 + (ps.p ? 1 : 0) + (ps.w ? 1 : 0)) * static_cast<double>(np) > 288.0 * 1048576.0;
  }
  return m;
}

MomentsPlan moments_plan_exact(int nx, int which, int deltaf, int64_t np, int num_cu) {
  MomentsPlan m = moments_plan(nx, which, deltaf, np, num_cu);   // (a 64-bit word per (plane, cell): the bytes are the doubles')
  // the exact diagnostics' rule (diag_launch, kind 1): a workgroup's final flush costs what a few trips cost
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(num_cu, (np + (int64_t{1} << 17) - 1) >> 17));
  for (int i = 0; i < m.npass; ++i) m.pass[i].blocks = static_cast<int>(blocks);
  return m;
}

PowerPlan power_plan(int nx, int nx_opd, int nv_opd, int which, int deltaf, int64_t np, int num_cu) {
  PowerPlan m{};
  if (which < 1 || which > 3 || ((which & 2) && !deltaf) || nx < 1 || nx_opd < 1 || nv_opd < 2) return m;
  m.tile = power_tile_bytes(nx);
  m.plane = sizeof(double) * static_cast<size_t>(nx_opd) * static_cast<size_t>(nv_opd);
  if (m.tile > kDiagLdsCap) return m;
  m.selected = which == 3 ? 2 : 1;
  const bool all_fit = m.tile + m.selected * m.plane <= kDiagLdsCap;
  const bool one_fits = m.tile + m.plane <= kDiagLdsCap;
  m.npass = all_fit || !one_fits ? 1 : m.selected;
  const int per_pass = m.selected / m.npass;
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(num_cu, ((np >> 1) + 1023) / 1024));
  for (int i = 0; i < m.npass; ++i) {
    PowerPass &ps = m.pass[i];
    ps.first_set = i * per_pass;
    ps.sets = per_pass;
    ps.p = per_pass == 2 || (which != 2 && i == 0);
    ps.w = per_pass == 2 || which == 2 || i == 1;
    ps.lds = one_fits;
    ps.threads = 1024;
    ps.blocks = static_cast<int>(blocks);
    ps.bytes = m.tile + (ps.lds ? per_pass * m.plane : 0);
    ps.nt = 8.0 * (2 + per_pass) * static_cast<double>(np) > 288.0 * 1048576.0;
  }
  return m;
}

PowerPlan power_plan_exact(int nx, int nx_opd, int nv_opd, int which, int deltaf, int64_t np, int num_cu) {
  PowerPlan m = power_plan(nx, nx_opd, nv_opd, which, deltaf, np, num_cu);   // (a 64-bit word per (set, bin): the bytes are the doubles')
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(num_cu, (np + (int64_t{1} << 17) - 1) >> 17));   // moments_plan_exact's rule
  for (int i = 0; i < m.npass; ++i) m.pass[i].blocks = static_cast<int>(blocks);
  return m;
}

HermitePlan hermite_plan(int nherm, int nmodes, int which, int deltaf, int64_t np, int num_cu) {
  HermitePlan h{};
  const int sets = which == 3 ? 2 : 1;
  if (which < 1 || which > 3 || ((which & 2) && !deltaf) || nherm < 1 || nherm > HERM_MAX_N || nmodes < 1 ||
      sets * nmodes > HERM_MAX_MODES || np < 0 || num_cu < 1)
    return h;
  h.threads = 256;
  const int waves = h.threads / 64;
  h.nb = nherm <= 64 ? 4 : (nherm <= 128 ? 8 : 16);
  h.bytes = HERM_WAVE_LDS * static_cast<size_t>(waves);
  // two workgroups fit a CU's LDS; a workgroup gets at least sixteen trips per wave before another one is started
  const int64_t chunks = (np + 63) >> 6, per_block = static_cast<int64_t>(waves) * kHermiteMinTrips;
  h.blocks = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(2 * static_cast<int64_t>(num_cu), (chunks + per_block - 1) / per_block)));
  h.nt = 8.0 * (2 + sets) * static_cast<double>(np) > 288.0 * 1048576.0;
  h.partials = static_cast<int64_t>(h.blocks) * (waves + 1);
  return h;
}

ZoomPlan zoom_plan(int nxb, int nvb, int which, int deltaf, int64_t np, int num_cu, int pass_cap) {
  ZoomPlan m{};
  if (which < 1 || which > 7 || ((which & 4) && !deltaf) || nxb < 1 || nvb < 1 || nxb > ZOOM_MAX_BINS || nvb > ZOOM_MAX_BINS ||
      static_cast<int64_t>(nxb) * nvb > ZOOM_MAX_CELLS)
    return m;
  m.selected = (which & 1) + ((which >> 1) & 1) + ((which >> 2) & 1);
  const int cap_words = static_cast<int>(kDiagLdsCap / sizeof(long long));
  const int rows_fit = cap_words / (m.selected * nxb);   // >= 1: a row of three planes is at most 12 288 words
  const int bands = (nvb + rows_fit - 1) / rows_fit;
  const bool lds = bands <= std::max(1, std::min(pass_cap, ZOOM_MAX_PASSES));
  m.npass = lds ? bands : 1;
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(num_cu, (np + (int64_t{1} << 17) - 1) >> 17));   // moments_plan_exact's rule
  for (int i = 0; i < m.npass; ++i) {
    ZoomPass &ps = m.pass[i];
    ps.lds = lds;
    ps.planes = which;
    ps.first_row = lds ? i * rows_fit : 0;
    ps.rows = lds ? std::min(rows_fit, nvb - ps.first_row) : nvb;
    ps.bytes = lds ? sizeof(long long) * static_cast<size_t>(m.selected) * ps.rows * nxb : 0;
    ps.threads = 1024;
    ps.blocks = static_cast<int>(blocks);
    ps.nt = 8.0 * (2 + ((which >> 1) & 1) + ((which >> 2) & 1)) * static_cast<double>(np) > 288.0 * 1048576.0;
  }
  return m;
}

SelectPlan select_plan(int64_t np, int num_cu, int threads_req, int bpc_req) {
  SelectPlan s{};
  s.chunk_pairs = SELECT_CHUNK_PAIRS;
  const int64_t npair = np > 0 ? np >> 1 : 0;
  s.nchunk = np > 0 ? std::max<int64_t>(1, (npair + s.chunk_pairs - 1) / s.chunk_pairs) : 0;
  s.threads = threads_req > 0 && threads_req <= 1024 && threads_req % 64 == 0 ? threads_req : 64;
  const int bpc = bpc_req > 0 ? bpc_req : 24;
  s.blocks = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(static_cast<int64_t>(num_cu) * bpc, s.nchunk)));
  s.nt = 16.0 * static_cast<double>(np) > 288.0 * 1048576.0;
  s.scan_threads = 1024;
  return s;
}

DigestLaunch digest_launch(int64_t nalloc, int num_cu) {
  DigestLaunch d{};
  d.threads = 256;
  d.nt = 32.0 * static_cast<double>(nalloc) > 288.0 * 1048576.0;
  const int64_t npair = (nalloc + 1) >> 1;
  d.blocks = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(static_cast<int64_t>(num_cu) * 8, (npair + d.threads - 1) / d.threads)));
  return d;
}

LoadLaunch load_launch(int64_t nalloc, int num_cu) {
  LoadLaunch l{};
  l.threads = 256;
  l.nt = 32.0 * static_cast<double>(nalloc) > 288.0 * 1048576.0;
  const int64_t nchunk = (nalloc + LOAD_CHUNK - 1) / LOAD_CHUNK;
  l.blocks = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(static_cast<int64_t>(num_cu) * 8, nchunk)));
  return l;
}

int64_t stream_plain_chunks(int64_t np_all_species, int64_t np_species, bool nt) {
  if (!nt || np_species <= 0 || np_all_species < np_species) return 0;
  // this species' share of the budget, in whole chunks of 64 pairs (4096 B of state)
  const double share = static_cast<double>(np_species) / static_cast<double>(np_all_species);
  const int64_t chunks = static_cast<int64_t>(share * static_cast<double>(kPlainStateBytes)) / 4096;
  return std::min(chunks, ((np_species >> 1) + 63) >> 6);  // (a slab within the budget: every chunk)
}

int tail_sum_blocks(int64_t ntail) {
  return ntail > 0 ? static_cast<int>(std::min<int64_t>(kEnergyBlocks, (ntail + 255) / 256)) : 0;
}

// fixed-point sums: a workgroup adds at most its share of the markers into one bin; weights <= 1
bool make_dist_scale(int64_t np, int blocks, bool deltaf, double bound_p, double bound_w, DistScale *out, int threads) {
  DistScale fx{};
  bool use_fx = blocks > 0 && bound_p > 0.0 && (!deltaf || bound_w > 0.0) && std::isfinite(bound_p) && std::isfinite(bound_w);
  if (use_fx) {
    const double th = static_cast<double>(threads);
    const double per_wg = 2.0 * th * std::ceil(static_cast<double>((np >> 1) + 1) / (static_cast<double>(blocks) * th)) + 2.0;
    const int e_n = static_cast<int>(std::ceil(std::log2(per_wg))) + 1;  // 2^e_n > the terms a bin can receive
    const double bounds[3] = {1.0, bound_p, deltaf ? bound_w : 1.0};
    for (int k = 0; k < 3; ++k) {
      int eb;
      (void)std::frexp(bounds[k], &eb);               // bounds[k] < 2^eb
      const int mag = std::min(62 - e_n, 50);         // |term * 2^e| < 2^mag: below 2^51 for to_fixed, and the sums below 2^62
      const int e = mag - eb;
      if (e < -900 || e > 900) use_fx = false;        // (a bound no scale can serve)
      fx.sc[k] = std::ldexp(1.0, e);
      fx.inv[k] = std::ldexp(1.0, -e);
      fx.bound[k] = std::ldexp(1.0, eb);
    }
  }
  *out = fx;
  return use_fx;
}

}  // namespace pic1dp
