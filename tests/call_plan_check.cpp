// call_plan_check.cpp -- a program of its own (tests/test_call_plan_host.py builds it with the host sanitizers and runs it):
// the call sites' state machine (pic1dp_amd/csrc/call_plan.cpp) walked COMPLETELY.  Breadth first from (Clean, Nothing,
// between time steps), through every kind of call under every combination of the moment's flags, for each of the cap sets
// below; at every state reached: the pair is legal, call_state_invariants holds, and every plan either succeeds or refuses
// with one of the codes the entry points had before the plan existed.  The moment's flags are free inputs here, so some
// (state, moment, call) triples cannot occur in a run: a refusal is accepted, and counted.  Prints, per cap set, the
// reachable (Seq, Owed) pairs and the number of refused triples; the last line is "<n> failed".
#include <cstdio>
#include <cstring>
#include <deque>
#include <set>
#include <string>
#include <vector>

#include "../pic1dp_amd/csrc/call_plan.cpp"

using namespace pic1dp;

namespace {

const char *const kSeq[] = {"Clean", "Push1", "Half", "HalfPair", "HalfPairSolved", "Push2", "Push2Pair", "Push2PairSolved"};
const char *const kOwed[] = {"Nothing", "Scale", "SumScale", "PredTiles", "PredSums", "AdoptHalfField"};

struct CapSet {
  const char *name;
  StepCaps k;
  CallMoment m;
};

// as step_caps derives them for a context whose whole-step kernels run (step_plan.cpp)
CapSet cap_set(const char *name, bool lazy, bool pair, int pred_kind, bool one_mode, bool predict, int charge_sum, bool several, int fuse_output) {
  CapSet c{name, StepCaps{}, CallMoment{}};
  const bool six = pred_kind == 2 && one_mode, capable = charge_sum == 0 && predict && pred_kind != 0;
  c.k.dft_paths = true, c.k.six_sums_one_mode = six, c.k.modes_fit_field_kernel = true, c.k.step_recompute_ok = true;
  c.k.predict_capable = capable;
  c.k.diag_in_step = charge_sum == 0 && (fuse_output == 2 || (fuse_output == 1 && !capable));
  c.k.lazy_calls_ok = lazy;
  c.k.pair_serves_collect = pair && lazy && !several && capable && six;
  c.k.pair_in_solve_field = pair && lazy && capable && six;
  c.m.lazy_calls = lazy, c.m.call_pair = pair, c.m.loaded = true, c.m.several_ranks = several;
  c.m.fp64_rank_sum = several && charge_sum == 0, c.m.charge_sum = charge_sum, c.m.pred_kind = pred_kind, c.m.tab_lds = true;
  return c;
}

long key_of(const CallState &s) {
  long k = static_cast<long>(s.seq);
  k = k * 8 + static_cast<long>(s.owed);
  k = k * 2 + s.e_step_start, k = k * 2 + s.cd_kept_mode_only, k = k * 2 + s.adopt_current;
  k = k * 2 + s.charge_pending, k = k * 2 + s.charge_pending_pred;
  k = k * 8 + s.call_phase, k = k * 4 + s.eh_modes;
  return k;
}

int walk(const CapSet &cs, std::set<std::string> &reached_all) {
  int failed = 0;
  long plans = 0, refused = 0;
  std::set<long> seen;
  std::set<std::string> pairs;
  std::deque<CallState> todo;
  todo.push_back(CallState{});
  seen.insert(key_of(todo.front()));
  auto fail = [&](const char *what, const CallState &s, int call, int flags) {
    if (++failed <= 5)
      std::printf("  FAILED %s: %s from (%s, %s) phase %d, call %s, flags %d\n", cs.name, what, kSeq[static_cast<int>(s.seq)],
                  kOwed[static_cast<int>(s.owed)], s.call_phase, call < 0 ? "-" : call_name(static_cast<Call>(call)), flags);
  };
  while (!todo.empty()) {
    const CallState s = todo.front();
    todo.pop_front();
    pairs.insert(std::string(kSeq[static_cast<int>(s.seq)]) + "/" + kOwed[static_cast<int>(s.owed)]);
    if (s.seq >= Seq::N || s.owed >= Owed::N || !kCallStateLegal[static_cast<int>(s.seq)][static_cast<int>(s.owed)]) fail("an illegal pair", s, -1, 0);
    if (const char *broken = call_state_invariants(s, cs.m, cs.k)) fail(broken, s, -1, 0);
    for (int call = 0; call < static_cast<int>(Call::N); ++call)
      for (int flags = 0; flags < 64; ++flags) {
        CallMoment m = cs.m;
        m.field_differs = flags & 1, m.pred_usable = flags & 2, m.eh_current = flags & 4, m.modes_current = flags & 8;
        m.optimize_due_any = flags & 16, m.output_follows = flags & 32;
        if (m.pred_usable && !cs.k.predict_capable) continue;  // (pred_usable implies predict_capable by its definition)
        const CallPlan p = plan_call(s, m, cs.k, static_cast<Call>(call));
        ++plans;
        if (p.refusal != Refusal::None) {
          ++refused;
          if (p.refusal >= Refusal::PlanTooLong) fail("a refusal the entry points did not have", s, call, flags);
          if (!p.refused_after) {
            if (p.n != 0 || !(p.next == s)) fail("a refused plan that does something", s, call, flags);
            continue;
          }
        }
        if (p.n > kMaxActs) fail("more actions than the plan holds", s, call, flags);
        if (seen.insert(key_of(p.next)).second) todo.push_back(p.next);
      }
  }
  std::printf("%s: %zu states, %ld plans, %ld refused\n  reachable:", cs.name, seen.size(), plans, refused);
  for (const std::string &p : pairs) std::printf(" %s", p.c_str()), reached_all.insert(p);
  std::printf("\n");
  return failed;
}

}  // namespace

int main() {
  const CapSet sets[] = {
      cap_set("six_sums_one_rank", true, true, 2, true, true, 0, false, 0),
      cap_set("six_sums_pair_off", true, false, 2, true, true, 0, false, 0),
      cap_set("tiles", true, true, 1, false, true, 0, false, 0),
      cap_set("no_prediction", true, true, 2, true, false, 0, false, 1),
      cap_set("exact_charge_sum", true, true, 2, true, true, 1, false, 0),
      cap_set("several_ranks", true, true, 2, true, true, 0, true, 0),
      cap_set("eager_call_sites", false, true, 2, true, true, 0, false, 0),
  };
  int failed = 0;
  std::set<std::string> reached;
  for (const CapSet &cs : sets) failed += walk(cs, reached);
  std::printf("reachable in all: %zu pairs:", reached.size());
  for (const std::string &p : reached) std::printf(" %s", p.c_str());
  std::printf("\n%d failed\n", failed);
  return failed != 0;
}
