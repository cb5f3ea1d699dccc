// settings.cpp -- the environment of a context, read in one place (settings.hpp).  No HIP call.
#include "settings.hpp"

#include <algorithm>
#include <cstdlib>

#include "kernels.hpp"

namespace pic1dp {

Settings settings_from_env() {
  Settings s;
  // ---- product variables ----
  if (const char *e = std::getenv("PIC1DP_FUSE_SOLVE")) s.fuse_solve = std::max(0, std::min(2, std::atoi(e)));
  if (const char *e = std::getenv("PIC1DP_TAIL")) s.tail_on = std::atoi(e) != 0;
  if (const char *e = std::getenv("PIC1DP_CALL_PAIR")) s.call_pair = std::atoi(e) != 0;
  if (const char *e = std::getenv("PIC1DP_LAZY_CALLS")) s.lazy_calls = std::atoi(e) != 0;
  if (const char *e = std::getenv("PIC1DP_PREDICT")) s.predict = std::atoi(e);
  if (const char *e = std::getenv("PIC1DP_DIAG_FX")) s.diag_fx = std::atoi(e) != 0;
  if (const char *e = std::getenv("PIC1DP_DIAG_FX_MARGIN")) s.diag_fx_margin_w = std::atof(e);
  if (const char *e = std::getenv("PIC1DP_PRED_KIND")) s.pred_kind_req = std::atoi(e);
  if (const char *e = std::getenv("PIC1DP_CHAIN_MFMA")) {  // 0 keeps the chain of additions in one lane, > 0 insists on the matrix unit
    const int k = std::atoi(e);
    s.chain_mfma_req = k == 0 ? 0 : (k > 0 ? 1 : -1);
  }
  // ---- tuning builds only ----
  if (const char *e = tuning_env("PIC1DP_OSUB")) s.osub_req = std::max(0, std::atoi(e));
  if (const char *e = tuning_env("PIC1DP_DYN_TAIL")) s.dyn_tail = s.dyn_tail_full = std::max(0, std::min(16, std::atoi(e)));
  if (const char *e = tuning_env("PIC1DP_DYN_TAIL_FULL")) s.dyn_tail_full = std::max(0, std::min(16, std::atoi(e)));
  if (const char *e = tuning_env("PIC1DP_NT_THRESHOLD_MB")) s.nt_threshold_half = s.nt_threshold_full = std::atof(e) * 1048576.0;
  if (const char *e = tuning_env("PIC1DP_NT_THRESHOLD_FULL_MB")) s.nt_threshold_full = std::atof(e) * 1048576.0;
  if (const char *e = tuning_env("PIC1DP_CARRY")) s.carry = std::max(0, std::atoi(e));
  if (const char *e = tuning_env("PIC1DP_RHO_GLOBAL_COPIES")) s.gcopies_req = accepted_gcopies(std::atoi(e));
  if (const char *e = tuning_env("PIC1DP_FIELD_ONE_RANK_ORDER")) s.field_one_rank_order = std::atoi(e) != 0;
  if (const char *e = tuning_env("PIC1DP_CHAIN_SELFTEST_VERBOSE")) s.chain_selftest_verbose = std::atoi(e) != 0;
  return s;
}

}  // namespace pic1dp
