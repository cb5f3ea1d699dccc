// select_host.cpp -- the host-only entry points of the marker selection (include/pic1dp_hip.h): the rule on host arrays
// (pic1dp_hip_host_select) and the thinning threshold of a fraction (pic1dp_hip_select_thin).  No HIP call, no context: the
// unit needs the header, select_rule.hpp and the library's error convention alone (tests/select_check.cpp builds it by
// itself under the host sanitizers).
#include "select_rule.hpp"

namespace pic1dp_host {
int fail(int code, const char *fmt, ...);   // ctx.hpp; capi.cpp
}

using namespace pic1dp;
using pic1dp_host::fail;

extern "C" {

int pic1dp_hip_select_thin(double fraction, uint64_t *thin) {
  if (!thin) return fail(PIC1DP_ERR_ARG, "select_thin: null output");
  uint64_t t = 0;
  if (!select_thin_of(fraction, &t)) return fail(PIC1DP_ERR_ARG, "select_thin: fraction = %g, must be > 0 (>= 1 keeps every marker)", fraction);
  *thin = t;
  return 0;
}

int pic1dp_hip_host_select(const pic1dp_input *in, const pic1dp_select *sel, const double *x, const double *v, int64_t np,
                           int64_t max, int64_t *count, int64_t *index) {
  if (!in || !sel || !count) return fail(PIC1DP_ERR_ARG, "host_select: null input, selection or count");
  if (np < 0 || max < 0) return fail(PIC1DP_ERR_ARG, "host_select: np = %lld, max = %lld: neither may be negative", (long long)np, (long long)max);
  if (np > 0 && (!x || !v)) return fail(PIC1DP_ERR_ARG, "host_select: null marker array");
  if (const char *why = select_refusal(*sel)) return fail(PIC1DP_ERR_ARG, "host_select: %s", why);
  int64_t n = 0;
  for (int64_t i = 0; i < np; ++i) {
    if (!select_keeps(*sel, in->lx, x[i], v[i], i)) continue;
    if (index && n < max) index[n] = i;
    ++n;
  }
  *count = n;
  return 0;
}

}  // extern "C"
