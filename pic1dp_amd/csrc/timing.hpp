// timing.hpp -- the event spans around launches and what they add up to: the reference's timers (ids < 100, iwt of
// include/pic1dp_hip.h) and the per-kernel statistics (tags >= 100).  A context holds one Timing (pic1dp_ctx::tm); the entry
// points that switch, read and reset it are capi_timing.cpp's.  Span is on the step path and stays inline.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/pic1dp_hip.h"

namespace pic1dp_host {

int fail(int code, const char *fmt, ...);  // (ctx.hpp: the error convention)

constexpr int kTagFused = 100, kTagPush = 101, kTagDeposit = 102, kTagStepHalf = 103, kTagStepFull = 104, kTagStepOne = 106,
              kTagMoments = 107, kTagMomentsExact = 108, kTagLoad = 109, kTagPower = 110, kTagSelect = 111, kTagGather = 112, kTagPowerExact = 113, kTagZoom = 114, kTagHermite = 115, kNumTags = 128;

struct EvPair {
  hipEvent_t a, b;
  int tag;
  bool head;  // one of the first 64 spans of its timer id since the last reset (sampled timers: taken as they are, not scaled)
};

// what the marker kernel launched last under a tag moves per marker (pic1dp_hip_kernel_bytes)
struct KernelBytes {
  double rd = 0.0, wr = 0.0, carry = 0.0;
  char name[64] = {0};
};

struct Timing {
  hipStream_t st = nullptr;  // the context's stream: where the events are recorded (set by create())
  bool timers_on = false, stats_on = false;
  std::vector<EvPair> evpool;
  size_t ev_used = 0;
  double acc_ms[kNumTags] = {0};
  int64_t acc_n[kNumTags] = {0};
  // timers (tags < 100) may be SAMPLED: only every timer_every-th block of 64 spans of a tag is bracketed by events (an event pair costs
  // the stream ~3 us of dependency: 10-28 % of a 70 us step at the reference's default size), the others only counted;
  // pic1dp_hip_timer_ms scales the sampled time by spans seen / spans timed
  int timer_every = 1;
  int64_t span_seen[kNumTags] = {0};
  // the first block of a timer id (first launches: code loading, cold caches, the run's first step) is always timed and
  // enters as it is; only the later blocks stand for the ones between them
  double head_ms[kNumTags] = {0};
  int64_t head_n[kNumTags] = {0};
  KernelBytes kbytes[kNumTags];
};

// the recorded pairs become milliseconds in acc_ms / head_ms: one stream synchronisation, none when nothing is recorded
// (capi_timing.cpp)
int ev_resolve(Timing &t);

// bracket helper: records a start event on construction (if enabled) and the
// stop event in end(); pairs are resolved to milliseconds lazily (ev_resolve)
struct Span {
  Timing &t;
  long idx = -1;
  int rc = 0;
  Span(Timing &t_, int tag, bool on) : t(t_) {
    if (!on) return;
    // sampled timers: blocks of 64 consecutive spans of a timer id are timed, every timer_every-th block -- inside a block
    // everything is bracketed as with exact timers (a run's output steps, optimisation steps and plain steps enter in
    // their own proportions), the other blocks are only counted
    const int64_t seq = tag < 100 ? t.span_seen[tag]++ : 0;
    if (tag < 100 && ((seq >> 6) % t.timer_every) != 0) return;
    if (t.ev_used == t.evpool.size() && t.evpool.size() >= (1u << 16)) {
      // a long run that reads its timers only at the end: fold what has been recorded into
      // the accumulators (one stream synchronisation per 65 536 spans) and reuse the pool
      if ((rc = ev_resolve(t)) != 0) return;
    }
    if (t.ev_used == t.evpool.size()) {
      EvPair p{};
      // timing only (the pairs are read after a stream synchronisation): no system-scope fence at the event -- with it
      // every bracketed launch pays a write-back of the caches its markers live in (a 70 us step at the reference's default
      // size: +10-28 %), and the time it reports contains that write-back
      // (A/B at the reference's default size: profiles/r05/experiments, tools/ab_event_fence.sh of that round)
      auto make = [](hipEvent_t *e) {
        if (hipEventCreateWithFlags(e, hipEventDisableSystemFence) == hipSuccess) return true;
        (void)hipGetLastError();
        return hipEventCreate(e) == hipSuccess;
      };
      if (!make(&p.a) || !make(&p.b)) {
        rc = fail(PIC1DP_ERR_HIP, "hipEventCreate failed");
        return;
      }
      t.evpool.push_back(p);
    }
    idx = static_cast<long>(t.ev_used++);
    t.evpool[idx].tag = tag;
    t.evpool[idx].head = tag < 100 && t.timer_every > 1 && seq < 64;
    if (hipEventRecord(t.evpool[idx].a, t.st) != hipSuccess) rc = fail(PIC1DP_ERR_HIP, "hipEventRecord failed");
  }
  int end() {
    if (idx >= 0 && hipEventRecord(t.evpool[idx].b, t.st) != hipSuccess)
      return fail(PIC1DP_ERR_HIP, "hipEventRecord failed");
    return rc;
  }
};

}  // namespace pic1dp_host
