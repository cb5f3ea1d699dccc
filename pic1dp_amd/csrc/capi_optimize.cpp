// capi_optimize.cpp -- marker optimisation events (particle_optimize -> particle_merge / particle_remove /
// particle_split, src/pic1dp_particle.F90:356-813).
#include <atomic>
#include <chrono>
#include <mutex>

#include "ctx.hpp"

namespace pic1dp_host {

// ---- marker optimisation (host side, rare; see optimize.hpp) -------------------
// which events are due for the step that is being taken: merge, remove, split
// time0: the time at the start of the step being taken
void optimize_due_at(const pic1dp_ctx *c, double time0, bool due[3]) {
  const pic1dp_input &in = c->in;
  const double t = time0 + in.dt;  // src/pic1dp_particle.F90:742,756,770
  due[0] = c->imerge > 0 && c->imerge <= in.nmerge && t >= in.tmerge[c->imerge - 1];
  due[1] = c->iremove > 0 && c->iremove <= in.nremove && t >= in.tremove[c->iremove - 1];
  due[2] = c->isplit > 0 && c->isplit <= in.nsplit && t >= in.tsplit[c->isplit - 1];
  if (in.deltaf == 0) due[0] = due[1] = due[2] = false;  // :734
}
void optimize_due(const pic1dp_ctx *c, bool due[3]) { optimize_due_at(c, c->time, due); }

bool optimize_due_any(const pic1dp_ctx *c) {
  bool due[3];
  optimize_due(c, due);
  return due[0] || due[1] || due[2];
}

// A worker's grow-only buffer.  Not the context owner's (device_mem.hpp): these grow on the workers' threads, and the
// owner is not thread-safe.
// Device scratch (DevBuf): grows when a block needs more than the ones before it (one hipMalloc / hipFree pair per worker
// and growth, not per block: round 5).
// Pinned host staging (HostPin): pageable copies on a worker's stream cost ~20 ms PER CALL here whatever their size (16
// blocks of 2.5 MB of keys: 335 ms, against 0.9 ms for the same blocks' 1-byte flags;
// profiles/r05/experiments/opt_event_bench_16_blocks.log), pinned ones what their bytes cost
template <bool Pinned>
struct GrowBuf {
  void *p = nullptr;
  size_t cap = 0;
  static void give_back(void *q) { Pinned ? (void)hipHostFree(q) : (void)hipFree(q); }
  ~GrowBuf() { give_back(p); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    give_back(p);
    p = nullptr;
    cap = 0;
    const size_t want = Pinned ? bytes + bytes / 8 + 64 : (bytes ? bytes + bytes / 8 : 16);
    const hipError_t e = Pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  template <class T>
  T *as() const { return static_cast<T *>(p); }
};
using DevBuf = GrowBuf<false>;
using HostPin = GrowBuf<true>;

using Clock = std::chrono::steady_clock;
static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// what one block worker of an event owns; created when an event first needs it, kept in the context until destroy()
// (streams, pinned and device allocations cost milliseconds each and synchronise the device: sixteen workers setting
// themselves up per event cost more than the walks they shared at 1e7 markers)
struct OptWorker {
  hipStream_t st = nullptr;
  DevBuf d_key, d_lists, d_holes;
  HostPin pin_up, pin_down;
  int64_t pcie = 0;                  // bytes moved between host and device, and the wall clock of the phases -- keys to the
  double tph[3] = {0.0, 0.0, 0.0};   // host | the walks | lists back + apply --, since run_blocks collected them last
  Clock::time_point t0;              // the stopwatch: start() ... lap(phase)
  ~OptWorker() {
    if (st) (void)hipStreamDestroy(st);
  }
  void start() { t0 = Clock::now(); }
  void lap(int phase) { tph[phase] += ms_since(t0), t0 = Clock::now(); }
  // THE transfers of an event, through the worker's pinned staging.  Up: every call drains the stream, so the staging is
  // free again when it returns
  hipError_t up(void *dst, const void *src, size_t bytes) {
    pcie += static_cast<int64_t>(bytes);
    if (!bytes) return hipSuccess;
    hipError_t e = pin_up.reserve(bytes);
    if (e != hipSuccess) return e;
    std::memcpy(pin_up.p, src, bytes);
    e = hipMemcpyAsync(dst, pin_up.p, bytes, hipMemcpyHostToDevice, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
  }
  // ... and down: *host points into the staging until the next down()
  hipError_t down(const void **host, const void *src, size_t bytes) {
    pcie += static_cast<int64_t>(bytes);
    hipError_t e = pin_down.reserve(bytes);
    if (e != hipSuccess) return e;
    *host = pin_down.p;
    if (!bytes) return hipSuccess;
    e = hipMemcpyAsync(pin_down.p, src, bytes, hipMemcpyDeviceToHost, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
  }
};

void optimize_release(pic1dp_ctx *c) {
  for (OptWorker *w : c->opt_workers) delete w;
  c->opt_workers.clear();
}

namespace {

int &event_counter(pic1dp_ctx *c, int kind) { return kind == 0 ? c->imerge : kind == 1 ? c->iremove : c->isplit; }
double event_threshold(pic1dp_ctx *c, int kind) {
  const double *th = kind == 0 ? c->in.thshmerge : kind == 1 ? c->in.thshremove : c->in.thshsplit;
  return th[event_counter(c, kind) - 1];
}

// particle_compute_dist_pertb_abs_v into hist[nspecies][nv]: block by block, summed in block order, then over processes
// (MPI_Allreduce, :356-403) -- THE statement of the reference's order of additions, whichever pass asks.
// contribution(s, b, local): block b's |delta f|(v) of species s into local[nv]; returns an error code
template <class Contribution>
int dist_pertb_abs_v(pic1dp_ctx *c, std::vector<double> &hist, Contribution contribution) {
  const int ns = c->in.nspecies, nb = c->plan.nblk, nv = c->in.nv;
  std::vector<double> local(nv);
  for (int s = 0; s < ns; ++s) {
    double *h = &hist[static_cast<size_t>(s) * nv];
    for (int b = 0; b < nb; ++b) {
      if (int rc = contribution(s, b, local.data())) return rc;
      for (int i = 0; i < nv; ++i) h[i] = b == 0 ? local[i] : h[i] + local[i];
    }
  }
  if (several_ranks(c)) {
    double *d = c->d_scratch;
    if (static_cast<size_t>(ns) * nv > static_cast<size_t>(kEnergyBlocks) * 3)
      return fail(PIC1DP_ERR_ARG, "nv too large for the reduction scratch");
    HIP_TRY(hipMemcpy(d, hist.data(), sizeof(double) * ns * nv, hipMemcpyHostToDevice));
    if (int rc = allreduce_doubles(c, d, static_cast<size_t>(ns) * nv)) return rc;
    HIP_TRY(hipStreamSynchronize(c->st));
    HIP_TRY(hipMemcpy(hist.data(), d, sizeof(double) * ns * nv, hipMemcpyDeviceToHost));
  }
  return 0;
}

// ---- the event with the markers staying on the device, kind by kind: keys -> walk -> lists -> apply ----
// |delta f|(v) of the block's species on the device, its peak, and the event's limit = peak * threshold
struct DfHist {
  const double *dev;
  double peak, limit;
};

// the moved markers' ids travel; the holes they move into are found on the device (opt_holes).  d_lists = pos[nm], id[nm],
// and -- 16-byte aligned -- `extra` bytes of the caller's
struct MoveLists {
  uint32_t *pos, *id;
  char *extra;
  int64_t n;
};
int upload_moves(OptWorker &w, const OptMoves &m, size_t extra, MoveLists &l) {
  const size_t nm = m.id.size();
  HIP_TRY(w.d_lists.reserve(sizeof(uint32_t) * 2 * (nm + 2) + extra + 64));
  l.pos = w.d_lists.as<uint32_t>();
  l.id = l.pos + nm;
  l.extra = w.d_lists.as<char>() + ((sizeof(uint32_t) * 2 * nm + 15) & ~static_cast<size_t>(15));
  l.n = static_cast<int64_t>(nm);
  HIP_TRY(w.up(l.id, m.id.data(), sizeof(uint32_t) * nm));
  return 0;
}

// particle_merge: 4 B per marker down
int merge_block(OptWorker &w, const OptBlock &B, const OptGrid &g, const DfHist &H, int64_t &np) {
  const void *keys = nullptr;
  HIP_TRY(w.d_key.reserve(sizeof(uint32_t) * np));
  HIP_TRY(opt_merge_keys(B, g, H.dev, H.limit, np, w.d_key.as<uint32_t>(), w.st));
  HIP_TRY(w.down(&keys, w.d_key.p, sizeof(uint32_t) * np));
  w.lap(0);
  MergePlan plan;
  plan_merge(static_cast<const uint32_t *>(keys), np, static_cast<size_t>(g.nx) * g.nv * 2, plan);
  w.lap(1);
  const size_t npairs = plan.dst.size();
  MoveLists l;
  if (int rc = upload_moves(w, plan.moves, sizeof(uint32_t) * 2 * (npairs + 2) + sizeof(double) * 4 * npairs + 32, l)) return rc;
  double *d_scr = reinterpret_cast<double *>(l.extra);
  uint32_t *d_dst = reinterpret_cast<uint32_t *>(d_scr + 4 * npairs), *d_k = d_dst + npairs;
  HIP_TRY(w.up(d_dst, plan.dst.data(), sizeof(uint32_t) * npairs));
  HIP_TRY(w.up(d_k, plan.idk.data(), sizeof(uint32_t) * npairs));
  HIP_TRY(w.d_holes.reserve(opt_holes_scratch_bytes(plan.np_new)));
  HIP_TRY(opt_holes(d_k, static_cast<int64_t>(npairs), nullptr, plan.np_new, l.n, l.pos, w.d_holes.p, w.st));
  HIP_TRY(opt_merge_apply(B, g, H.dev, H.limit, d_dst, d_k, static_cast<int64_t>(npairs), l.pos, l.id, l.n, plan.moves.ghost,
                          plan.np_new, d_scr, w.st));
  np = plan.np_new;
  return 0;
}

// particle_remove: 8 B (typeremove 2) or 1 B (typeremove 1) per marker down; continues the block's random stream
int remove_block(OptWorker &w, const OptBlock &B, const OptGrid &g, const DfHist &H, const pic1dp_input &in, Multirand &rng,
                 int64_t &np) {
  const int by_threshold = in.typeremove == 1 ? 1 : 0;
  const size_t bytes = (by_threshold ? sizeof(uint8_t) : sizeof(double)) * np;
  const void *vals = nullptr;
  HIP_TRY(w.d_key.reserve(bytes));
  HIP_TRY(opt_remove_vals(B, g, H.dev, H.peak, H.limit, by_threshold, np, w.d_key.as<uint8_t>(), w.d_key.as<double>(), w.st));
  HIP_TRY(w.down(&vals, w.d_key.p, bytes));
  w.lap(0);
  RemovePlan plan;
  plan_remove(in, by_threshold ? static_cast<const uint8_t *>(vals) : nullptr, by_threshold ? nullptr : static_cast<const double *>(vals),
              rng, np, plan);
  w.lap(1);
  MoveLists l;
  if (int rc = upload_moves(w, plan.moves, sizeof(uint32_t) * (plan.gone_bits.size() + 4), l)) return rc;
  uint32_t *d_bits = reinterpret_cast<uint32_t *>(l.extra);
  HIP_TRY(w.up(d_bits, plan.gone_bits.data(), sizeof(uint32_t) * plan.gone_bits.size()));
  HIP_TRY(w.d_holes.reserve(opt_holes_scratch_bytes(plan.np_new)));
  HIP_TRY(opt_holes(nullptr, 0, d_bits, plan.np_new, l.n, l.pos, w.d_holes.p, w.st));
  HIP_TRY(opt_remove_apply(B, g, H.dev, H.peak, H.limit, by_threshold, 1.0 - in.remove_frac, l.pos, l.id, l.n, plan.moves.ghost,
                           plan.np_new, w.st));
  np = plan.np_new;
  return 0;
}

// particle_split: 1 B per marker down; continues the block's random stream
int split_block(OptWorker &w, const OptBlock &B, const OptGrid &g, const DfHist &H, const pic1dp_input &in, Multirand &rng,
                int64_t nalloc, int64_t &np) {
  const void *flag = nullptr;
  HIP_TRY(w.d_key.reserve(sizeof(uint8_t) * np));
  HIP_TRY(opt_split_flags(B, g, H.dev, H.limit, np, w.d_key.as<uint8_t>(), w.st));
  HIP_TRY(w.down(&flag, w.d_key.p, sizeof(uint8_t) * np));
  w.lap(0);
  SplitPlan plan;
  plan_split(in, static_cast<const uint8_t *>(flag), rng, nalloc, np, plan);
  w.lap(1);
  const size_t nsp = plan.ks.size();
  HIP_TRY(w.d_lists.reserve(sizeof(double) * plan.dv.size() + sizeof(uint32_t) * nsp + 64));
  double *d_dv = w.d_lists.as<double>();
  uint32_t *d_ks = reinterpret_cast<uint32_t *>(d_dv + plan.dv.size());
  HIP_TRY(w.up(d_ks, plan.ks.data(), sizeof(uint32_t) * nsp));
  HIP_TRY(w.up(d_dv, plan.dv.data(), sizeof(double) * plan.dv.size()));
  HIP_TRY(opt_split_apply(B, np, d_ks, d_dv, static_cast<int64_t>(nsp), in.split_ngroup, in.deltaf, w.st));
  np = plan.np_new;
  return 0;
}

// what the blocks of one kind of event share
struct Event {
  int kind;
  double threshold;
  OptGrid grid;
  const std::vector<std::vector<OptBlock>> &ob;  // [nspecies][nblk] the layout the event began with
  const double *hist, *d_hist;                   // [nspecies][nv] |delta f|(v), on the host and on the device
};

// one reference block: its species in order (they share the block's random stream)
int event_block(pic1dp_ctx *c, OptWorker &w, const Event &ev, int b) {
  const int nv = ev.grid.nv;
  for (int s = 0; s < c->in.nspecies; ++s) {
    int64_t &np = c->blk_np[s][b];
    if (np <= 0) continue;
    const double *h = ev.hist + static_cast<size_t>(s) * nv;
    const double peak = *std::max_element(h, h + nv);
    const DfHist H{ev.d_hist + static_cast<size_t>(s) * nv, peak, peak * ev.threshold};
    w.start();
    int rc = 0;
    if (ev.kind == 0) rc = merge_block(w, ev.ob[s][b], ev.grid, H, np);
    if (ev.kind == 1) rc = remove_block(w, ev.ob[s][b], ev.grid, H, c->in, c->blk_rng[b], np);
    if (ev.kind == 2) rc = split_block(w, ev.ob[s][b], ev.grid, H, c->in, c->blk_rng[b], c->plan.blk_alloc[b], np);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(w.st));  // (the lists are reused next)
    w.lap(2);
  }
  return 0;
}

// host threads of an event: one per block up to the host's cores and 16, or PIC1DP_OPT_THREADS; each with a worker
int event_workers(pic1dp_ctx *c, int *nthreads) {
  const int nb = c->plan.nblk;
  *nthreads = std::min<int>(nb, std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
  if (const char *e = std::getenv("PIC1DP_OPT_THREADS")) *nthreads = std::max(1, std::min(nb, std::atoi(e)));
  while (static_cast<int>(c->opt_workers.size()) < *nthreads) {
    c->opt_workers.push_back(new OptWorker());
    HIP_TRY(hipStreamCreateWithFlags(&c->opt_workers.back()->st, hipStreamNonBlocking));
  }
  return 0;
}

// The blocks of an event side by side: the reference's own blocks are independent -- one rank each in the reference, own
// random stream, own markers (src/pic1dp_particle.F90:411-746 run per rank) --, so nthreads workers draw block numbers
// from a counter, every one with a stream and scratch of its own.  block(worker, b) returns an error code; the first
// error's message is thread-local: handed to the caller's thread.  Same decisions, same bits, whatever nthreads.
// tph += the workers' phases: keys to the host | the walks | lists back + apply
template <class Block>
int run_blocks(pic1dp_ctx *c, int nthreads, double tph[3], Block block) {
  const int nb = c->plan.nblk;
  std::atomic<int> next{0};
  std::mutex err_mu;
  int err_rc = 0;
  std::string err_msg;
  auto worker = [&](int t) {
    OptWorker &w = *c->opt_workers[t];
    const hipError_t e = hipSetDevice(c->device);
    int rc = e == hipSuccess ? 0 : fail(PIC1DP_ERR_HIP, "optimisation worker: %s", hipGetErrorString(e));
    for (int b = next.fetch_add(1); rc == 0 && b < nb; b = next.fetch_add(1)) rc = block(w, b);
    (void)hipStreamSynchronize(w.st);
    if (rc == 0) return;
    std::lock_guard<std::mutex> lk(err_mu);
    if (err_rc == 0) err_rc = rc, err_msg = pic1dp_hip_last_error();
    next.store(nb);  // the others stop drawing
  };
  if (nthreads <= 1) {
    worker(0);
  } else {
    std::vector<std::thread> pool;
    for (int t = 0; t < nthreads; ++t) pool.emplace_back(worker, t);
    for (auto &t : pool) t.join();
  }
  for (OptWorker *w : c->opt_workers) {  // what they counted (worker 0: the caller's transfers before the run too)
    c->cnt.opt_pcie_bytes += w->pcie, w->pcie = 0;
    for (int k = 0; k < 3; ++k) tph[k] += w->tph[k], w->tph[k] = 0.0;
  }
  return err_rc ? fail(err_rc, "%s", err_msg.c_str()) : 0;
}

// re-pack into the other slab -- valid markers of all blocks first, their tail slots behind, as the layout wants them --
// and make it the species' storage
int repack(pic1dp_ctx *c, const std::vector<std::vector<OptBlock>> &ob) {
  for (int s = 0; s < c->in.nspecies; ++s) {
    Species &S = c->sp[s];
    const BlockLayout to = block_layout(c->plan.blk_alloc, c->blk_np[s]);
    std::swap(S.slab[0], S.slab[1]);
    wire_species(S, c->in);  // (the OptBlocks still name the slab the event ran in)
    for (int b = 0; b < c->plan.nblk; ++b) {
      const BlockSpan &T = to.blk[b];
      HIP_TRY(opt_copy_segment(ob[s][b], 0, T.np, S.set[0].x, S.set[0].v, S.p, S.set[0].w, T.voff, c->st));
      HIP_TRY(opt_copy_segment(ob[s][b], T.np, T.ntail, S.set[0].x, S.set[0].v, S.p, S.set[0].w, T.toff, c->st));
    }
    S.np = to.np;
    HIP_TRY(hipStreamSynchronize(c->st));
  }
  return 0;
}

// The event with the markers staying on the device (kernels_opt.hip): per block the |delta f|(v) histogram in the
// reference's order of additions, one small key per marker to the host, the sequential walk there (optimize.cpp
// plan_*: visiting order, swap-with-last, merge partners, the block's random stream), and what the walk decided back:
// moves, merge pairs, the split parents and their velocity offsets.  1-8 B per marker over PCIe plus the lists --
// instead of 64 B.  Bit for bit what opt_merge / opt_remove / opt_split leave (tests/test_gpu_optimize.py).
// The walk is what an event costs (round 4: 137-157 ms at 1e7 markers), hence run_blocks (round 5).
int optimize_on_device(pic1dp_ctx *c, const bool due[3]) {
  const pic1dp_input &in = c->in;
  const int ns = in.nspecies, nb = c->plan.nblk, nv = in.nv;
  if (int rc = ensure_second_set(c)) return rc;  // the re-packing target
  // PIC1DP_OPT_TIMING=1: wall clock of the event's phases to stderr (tools/opt_event_bench.py)
  const char *te = tuning_env("PIC1DP_OPT_TIMING");
  const bool timing = te && std::atoi(te) != 0;
  double t_hist = 0.0, t_blocks = 0.0;
  const OptGrid grid{in.lx, in.v_max, in.nx, nv};
  // the layout the event starts from; the histogram's sort scratch for its largest block (counts only shrink before the
  // last kind's histogram: a split comes last)
  std::vector<std::vector<OptBlock>> ob(ns, std::vector<OptBlock>(nb));
  size_t sort_bytes = 16;
  for (int s = 0; s < ns; ++s) {
    const Species &S = c->sp[s];
    const BlockLayout from = block_layout(c->plan.blk_alloc, c->blk_np[s]);
    for (int b = 0; b < nb; ++b) {
      ob[s][b] = OptBlock{S.set[0].x, S.set[0].v, S.p, S.set[0].w, from.blk[b].voff, from.blk[b].np, from.blk[b].toff};
      sort_bytes = std::max(sort_bytes, opt_hist_scratch_bytes(from.blk[b].np, nv));
    }
  }
  CallBuf<double> d_hist(c->mem), d_local(c->mem);
  CallBuf<char> d_sort(c->mem);
  if (int rc = d_hist.take(static_cast<size_t>(ns) * nv, "particle_optimize", "|delta f|(v)")) return rc;
  if (int rc = d_local.take(nv, "particle_optimize", "a block's |delta f|(v)")) return rc;
  if (int rc = d_sort.take(sort_bytes, "particle_optimize", "the histogram's sort")) return rc;
  int nthreads = 1;
  if (int rc = event_workers(c, &nthreads)) return rc;
  OptWorker &w0 = *c->opt_workers[0];  // (the caller's thread borrows its transfers between the blocks' runs)
  std::vector<double> hist(static_cast<size_t>(ns) * nv);
  for (int kind = 0; kind < 3; ++kind) {
    if (!due[kind]) continue;
    auto t_phase = Clock::now();
    int rc = dist_pertb_abs_v(c, hist, [&](int s, int b, double *local) -> int {
      const int64_t np = c->blk_np[s][b];
      if (opt_hist_scratch_bytes(np, nv) > sort_bytes) return fail(PIC1DP_ERR_STATE, "a block outgrew the histogram's sort scratch");
      const void *staged = nullptr;
      HIP_TRY(opt_hist_block(ob[s][b], grid, np, d_local.p, d_sort.p, c->st));
      HIP_TRY(w0.down(&staged, d_local.p, sizeof(double) * nv));
      std::memcpy(local, staged, sizeof(double) * nv);
      return 0;
    });
    if (rc) return rc;
    HIP_TRY(w0.up(d_hist.p, hist.data(), sizeof(double) * ns * nv));
    const Event ev{kind, event_threshold(c, kind), grid, ob, hist.data(), d_hist.p};
    t_hist += ms_since(t_phase);
    t_phase = Clock::now();
    double tph[3] = {0.0, 0.0, 0.0};
    rc = run_blocks(c, nthreads, tph, [&](OptWorker &w, int b) { return event_block(c, w, ev, b); });
    if (rc) return rc;
    t_blocks += ms_since(t_phase);
    if (timing)
      std::fprintf(stderr, "pic1dp:   summed over the workers: keys to the host %.1f ms, the walks %.1f ms, lists back + apply %.1f ms\n",
                   tph[0], tph[1], tph[2]);
    event_counter(c, kind) += 1;
  }
  const auto t_repack = Clock::now();
  if (int rc = repack(c, ob)) return rc;
  if (timing)
    std::fprintf(stderr, "pic1dp: optimisation event: |delta f|(v) %.1f ms, %d blocks on %d host threads %.1f ms, re-pack %.1f ms\n",
                 t_hist, nb, nthreads, t_blocks, ms_since(t_repack));
  return 0;
}

// every owned block of a species between the device and a host copy of its full allocation (valid markers + tail slots)
struct HostBlock {
  std::vector<double> a[4];  // x v p w
};
int move_blocks(pic1dp_ctx *c, int s, std::vector<HostBlock> &host, bool to_device) {
  Species &S = c->sp[s];
  double *dev[4] = {S.set[0].x, S.set[0].v, S.p, S.set[0].w};
  const BlockLayout L = block_layout(c->plan.blk_alloc, c->blk_np[s]);
  for (int b = 0; b < c->plan.nblk; ++b)
    for (int k = 0; k < 4; ++k) {
      const BlockSpan &B = L.blk[b];
      host[b].a[k].resize(static_cast<size_t>(B.np + B.ntail));
      double *h = host[b].a[k].data();
      if (int rc = to_device ? put_range(c, dev[k], B.voff, h, B.np) : get_range(c, dev[k], B.voff, h, B.np)) return rc;
      if (int rc = to_device ? put_range(c, dev[k], B.toff, h + B.np, B.ntail) : get_range(c, dev[k], B.toff, h + B.np, B.ntail)) return rc;
    }
  S.np = L.np;
  return 0;
}

// the event on host copies of the owned blocks (PIC1DP_OPT_HOST=1): every marker crosses PCIe twice, 64 B in all
int optimize_on_host(pic1dp_ctx *c, const bool due[3]) {
  const pic1dp_input &in = c->in;
  const int ns = in.nspecies, nb = c->plan.nblk, nv = in.nv;
  std::vector<std::vector<HostBlock>> host(ns, std::vector<HostBlock>(nb));
  for (int s = 0; s < ns; ++s)
    if (int rc = move_blocks(c, s, host[s], false)) return rc;
  std::vector<double> hist(static_cast<size_t>(ns) * nv);
  for (int kind = 0; kind < 3; ++kind) {
    if (!due[kind]) continue;
    int rc = dist_pertb_abs_v(c, hist, [&](int s, int b, double *local) -> int {
      std::fill(local, local + nv, 0.0);
      opt_histogram(in, c->blk_np[s][b], host[s][b].a[1].data(), host[s][b].a[3].data(), local);
      return 0;
    });
    if (rc) return rc;
    const double th = event_threshold(c, kind);
    for (int b = 0; b < nb; ++b)
      for (int s = 0; s < ns; ++s) {
        double *x = host[s][b].a[0].data(), *v = host[s][b].a[1].data(), *p = host[s][b].a[2].data(), *w = host[s][b].a[3].data();
        const double *h = &hist[static_cast<size_t>(s) * nv];
        int64_t &np = c->blk_np[s][b];
        if (kind == 0) opt_merge(in, th, h, np, x, v, p, w);
        if (kind == 1) opt_remove(in, th, h, c->blk_rng[b], np, x, v, p, w);
        if (kind == 2) opt_split(in, th, h, c->blk_rng[b], c->plan.blk_alloc[b], np, x, v, p, w);
      }
    event_counter(c, kind) += 1;
  }
  // back to the device: valid markers of all blocks packed first, tails behind
  for (int s = 0; s < ns; ++s)
    if (int rc = move_blocks(c, s, host[s], true)) return rc;
  for (int s = 0; s < ns; ++s) c->cnt.opt_pcie_bytes += 2 * 32 * c->sp[s].nalloc;
  return 0;
}

}  // namespace
}  // namespace pic1dp_host

extern "C" int pic1dp_hip_particle_optimize(pic1dp_ctx *c, int32_t irk, int32_t *flag_optimized) {
  CHECK_CTX(c);
  if (flag_optimized) *flag_optimized = 0;
  if (irk != 1 && irk != 2) return fail(PIC1DP_ERR_ARG, "irk must be 1 or 2");
  bool due[3];
  optimize_due(c, due);
  if (irk != 2 || !(due[0] || due[1] || due[2])) return 0;
  if (int rc = require_loaded(c)) return rc;
  if (c->cur != 0) return fail(PIC1DP_ERR_STATE, "particle_optimize must follow the push of sub-step 2");
  if ((due[1] || due[2]) && !c->rng_ready)
    return fail(PIC1DP_ERR_STATE,
                "particle_remove / particle_split continue the loader's random stream: load the markers with "
                "pic1dp_hip_particle_load");
  for (int s = 0; s < c->in.nspecies; ++s)
    if (block_layout(c->plan.blk_alloc, c->blk_np[s]).np != c->sp[s].np)
      return fail(PIC1DP_ERR_STATE, "marker counts per block unknown (uploaded over several blocks)");
  Span tm(c->tm, PIC1DP_IWT_PARTICLE_OPTIMIZE, c->tm.timers_on);
  c->state_version++;
  HIP_TRY(hipStreamSynchronize(c->st));
  const char *eh = std::getenv("PIC1DP_OPT_HOST");  // (read per event: rare)
  // the device path names positions inside a block with 32 bits (keys, move lists, bit masks): a block of 2^32 slots or
  // more -- 137 GB of markers in one reference block -- takes the host copies, which count in 64 bits
  const int64_t max_alloc = *std::max_element(c->plan.blk_alloc.begin(), c->plan.blk_alloc.end());
  const bool on_host = (eh && std::atoi(eh) != 0) || max_alloc >= (int64_t{1} << 32) - 2;
  if (int rc = on_host ? optimize_on_host(c, due) : optimize_on_device(c, due)) return rc;
  diag_void_bounds(c);  // (merged / rescaled / split weights)
  if (flag_optimized) *flag_optimized = 1;
  return tm.end();
}
