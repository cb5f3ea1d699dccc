// capi_select.cpp -- select and gather markers on the device behind the C ABI (include/pic1dp_hip.h pic1dp_hip_select_count,
// _select, _gather): passes of their own in the mould of capi_products.cpp, which cache nothing and change
// nothing.  Every device buffer of a call -- the chunk counts, the result, a gather's indices -- is taken from the context's
// owner and given back before the call returns; results cross to the host through the context's pinned staging in slices.
// The rule on the host and the thinning threshold are select_host.cpp's; the call's buffers and the sliced transfer (CallBuf,
// words_to_host) are ctx.hpp's, shared with capi_zoom.cpp.
#include <algorithm>

#include "ctx.hpp"
#include "select_rule.hpp"

namespace {

// ... and from the host to the device
int words_to_device(pic1dp_ctx *c, void *dev, const void *host, int64_t n) {
  if (n <= 0) return 0;
  double *h = nullptr;
  if (int rc = pinned(c, static_cast<size_t>(std::min(n, kSliceWords)), &h)) return rc;
  for (int64_t done = 0; done < n; done += kSliceWords) {
    const int64_t m = std::min(kSliceWords, n - done);
    std::memcpy(h, static_cast<const double *>(host) + done, sizeof(double) * m);
    HIP_TRY(hipMemcpyAsync(static_cast<double *>(dev) + done, h, sizeof(double) * m, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));   // (the staging is free for the next slice)
  }
  return 0;
}

SelectRule rule_of(const pic1dp_select &s, double lx) {
  SelectRule r{};
  r.lx = lx;
  r.x_lo = s.x_lo, r.x_hi = s.x_hi, r.v_lo = s.v_lo, r.v_hi = s.v_hi;
  r.thin = s.thin, r.key = s.key, r.origin = static_cast<unsigned long long>(s.origin);
  r.straddle = s.x_lo > s.x_hi ? 1 : 0;
  return r;
}

// where the valid markers of a species live now, and its tail slots (set 0: pic1dp_hip_particles_download)
SelectArrays current_arrays(const pic1dp_ctx *c, const Species &S) {
  const PSet &A = S.set[c->cur];
  return SelectArrays{A.x, A.v, S.p, A.w};
}
SelectArrays tail_arrays(const Species &S) { return SelectArrays{S.set[0].x, S.set[0].v, S.p, S.set[0].w}; }

// count, and where `max` > 0 and an output array is given, write: both entry points
int select_run(pic1dp_ctx *c, const char *who, int32_t isp, const pic1dp_select *sel, int64_t max, int64_t *count, int64_t *index,
               double *x, double *v, double *p, double *w) {
  CHECK_CTX(c);
  if (!sel || !count) return fail(PIC1DP_ERR_ARG, "%s: null selection or count", who);
  if (max < 0) return fail(PIC1DP_ERR_ARG, "%s: max = %lld is negative", who, (long long)max);
  if (const char *why = select_refusal(*sel)) return fail(PIC1DP_ERR_ARG, "%s: %s", who, why);
  if (int rc = product_begin(c, who, isp)) return rc;
  const Species &S = c->sp[isp];
  const SelectPlan plan = select_plan(S.np, c->num_cu, c->threads_req, c->bpc_req);
  if (plan.nchunk < 1) {   // no valid marker
    *count = 0;
    return 0;
  }
  const SelectRule rule = rule_of(*sel, c->in.lx);
  const SelectArrays arr = current_arrays(c, S);
  CallBuf<unsigned long long> counts(c->mem);
  if (int rc = counts.take(static_cast<size_t>(plan.nchunk) + 1, who, "the chunk counts")) return rc;
  {  // (count and scan: one span, one pass)
    Span ks(c->tm, kTagSelect, c->tm.stats_on);
    HIP_TRY(launch_select_count(arr, S.np, rule, counts.p, plan, c->st));
    HIP_TRY(launch_select_scan(counts.p, plan, c->st));
    if (int rc = ks.end()) return rc;
    c->cnt.select_passes++;
  }
  unsigned long long total = 0;
  if (int rc = words_to_host(c, &total, counts.p + plan.nchunk, 1)) return rc;
  const int64_t n = std::min(static_cast<int64_t>(total), max);
  void *const host[5] = {index, x, v, p, w};
  const bool any = index || x || v || p || w;
  if (n > 0 && any) {
    CallBuf<double> res(c->mem);   // [5][n]: index, x, v, p, w -- 40 B per marker handed out
    if (int rc = res.take(static_cast<size_t>(5) * static_cast<size_t>(n), who, "the selected markers")) return rc;
    double *d[5];
    for (int k = 0; k < 5; ++k) d[k] = host[k] ? res.p + static_cast<size_t>(k) * static_cast<size_t>(n) : nullptr;
    const SelectOut out{reinterpret_cast<long long *>(d[0]), d[1], d[2], d[3], d[4]};
    auto write = [&](int) { return launch_select_write(arr, S.np, rule, counts.p, n, out, plan, c->st); };
    if (int rc = run_passes(c, kTagSelect, c->cnt.select_passes, 1, S.np, write)) return rc;
    for (int k = 0; k < 5; ++k)
      if (int rc = words_to_host(c, host[k], d[k], n)) return rc;
  }
  *count = static_cast<int64_t>(total);
  return 0;
}

}  // namespace

extern "C" {

int pic1dp_hip_select_count(pic1dp_ctx *c, int32_t isp, const pic1dp_select *sel, int64_t *count) {
  return select_run(c, "select_count", isp, sel, 0, count, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int pic1dp_hip_select(pic1dp_ctx *c, int32_t isp, const pic1dp_select *sel, int64_t max, int64_t *count, int64_t *index, double *x,
                      double *v, double *p, double *w) {
  return select_run(c, "select", isp, sel, max, count, index, x, v, p, w);
}

int pic1dp_hip_gather(pic1dp_ctx *c, int32_t isp, const int64_t *index, int64_t n, double *x, double *v, double *p, double *w) {
  CHECK_CTX(c);
  if (n < 0) return fail(PIC1DP_ERR_ARG, "gather: n = %lld is negative", (long long)n);
  if (n == 0) return 0;
  if (!index) return fail(PIC1DP_ERR_ARG, "gather: null index array");
  if (int rc = product_check(c, "gather", isp)) return rc;
  const Species &S = c->sp[isp];
  for (int64_t k = 0; k < n; ++k)
    if (index[k] < 0 || index[k] >= S.nalloc)
      return fail(PIC1DP_ERR_ARG, "gather: index[%lld] = %lld lies outside [0, %lld), the slots of species %d", (long long)k,
                  (long long)index[k], (long long)S.nalloc, isp);
  if (int rc = product_begin(c, "gather", isp)) return rc;
  void *const host[4] = {x, v, p, w};
  if (!x && !v && !p && !w) return 0;
  CallBuf<long long> idx(c->mem);
  if (int rc = idx.take(static_cast<size_t>(n), "gather", "the indices")) return rc;
  CallBuf<double> res(c->mem);   // [4][n]: x, v, p, w
  if (int rc = res.take(static_cast<size_t>(4) * static_cast<size_t>(n), "gather", "the gathered markers")) return rc;
  if (int rc = words_to_device(c, idx.p, index, n)) return rc;
  double *d[4];
  for (int k = 0; k < 4; ++k) d[k] = host[k] ? res.p + static_cast<size_t>(k) * static_cast<size_t>(n) : nullptr;
  const SelectOut out{nullptr, d[0], d[1], d[2], d[3]};
  auto pass = [&](int) { return launch_gather(current_arrays(c, S), tail_arrays(S), S.np, idx.p, n, out, c->st); };
  if (int rc = run_passes(c, kTagGather, c->cnt.gather_launches, 1, n, pass)) return rc;
  for (int k = 0; k < 4; ++k)
    if (int rc = words_to_host(c, host[k], d[k], n)) return rc;
  return 0;
}

}  // extern "C"
