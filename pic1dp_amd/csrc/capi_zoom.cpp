// capi_zoom.cpp -- the exact phase-space histogram on a caller-chosen window and grid behind the C ABI (include/pic1dp_hip.h
// pic1dp_hip_zoom, _zoom_local_exact, _zoom_convert, _host_zoom, _zoom_len, _zoom_limbs_len): passes of
// their own in the mould of capi_products.cpp, which cache nothing and change nothing.  The device rows and the counters of a
// call are taken from the context's owner and given back before the call returns (ctx.hpp CallBuf), the limbs cross to the
// host through the context's pinned staging in slices.  The rule on the host, the checks and the limb arithmetic are
// zoom_fx.cpp's; the entry points that take no context make no HIP call.
#include "ctx.hpp"
#include "zoom_fx.hpp"

namespace {

const char *const kPlaneName[3] = {"markr", "total", "pertb"};

// the refusals every entry point shares, in this order: null arguments, which, pertb of a full-f run, the window and grid,
// the species; e: the log2 quanta of markr (0), total and pertb
int zoom_refusals(const char *who, const pic1dp_input *in, int32_t isp, const pic1dp_zoom *z, int32_t which, int32_t e[3]) {
  if (!in || !z) return fail(PIC1DP_ERR_ARG, "%s: null input or window", who);
  if (which < 1 || which > 7) return fail(PIC1DP_ERR_ARG, "%s: which = %d, must be a mask of 1 (markr), 2 (total) and 4 (pertb)", who, which);
  if ((which & 4) && in->deltaf == 0)
    return fail(PIC1DP_ERR_ARG, "%s: which = %d asks for the plane pertb (which & 4), but a full-f context (deltaf = 0) has no w", who, which);
  if (const char *why = zoom_refusal(*z, in->lx))
    return fail(PIC1DP_ERR_ARG, "%s: %s (x [%g, %g) in a box of %g, v [%g, %g), %d x %d cells)", who, why, z->x_lo, z->x_hi, in->lx, z->v_lo,
                z->v_hi, z->nxb, z->nvb);
  int32_t e6[6];
  if (int rc = pic1dp_hip_diag_quanta(in, isp, e6)) return rc;   // (the input's version and species index with it)
  e[0] = 0, e[1] = e6[1], e[2] = e6[2];
  return 0;
}

int zoom_pass_cap() {   // a measurement varies the cap (a tuning build alone looks; tools/zoom_bench.py)
  if (const char *s = tuning_env("PIC1DP_ZOOM_PASS_CAP")) return std::max(1, std::atoi(s));
  return kZoomPassCap;
}

// this context's exact sums of species isp into limbs (host memory of zoom_limbs_len words), normalised; terms not summed:
// counted, PIC1DP_ERR_ARG, nothing written
int zoom_local(pic1dp_ctx *c, const char *who, int32_t isp, const pic1dp_zoom *z, int32_t which, int64_t *limbs) {
  CHECK_CTX(c);
  int32_t e[3];
  if (int rc = zoom_refusals(who, &c->in, isp, z, which, e)) return rc;
  if (!limbs) return fail(PIC1DP_ERR_ARG, "%s: null output", who);
  if (int rc = product_begin(c, who, isp)) return rc;
  const Species &S = c->sp[isp];
  const ZoomGeom zg = zoom_geom(*z, c->in.lx);
  const size_t cells = static_cast<size_t>(z->nxb) * z->nvb, n = 2 * cells * zoom_planes(which);
  if (z->x_lo == z->x_hi || S.np <= 0) {   // the empty window, no valid marker: nothing is launched
    std::memset(limbs, 0, sizeof(int64_t) * n);
    return 0;
  }
  const ZoomPlan plan = zoom_plan(z->nxb, z->nvb, which, c->in.deltaf, S.np, c->num_cu, zoom_pass_cap());
  if (plan.npass < 1) return fail(PIC1DP_ERR_STATE, "internal: zoom_plan has no pass for %d x %d, which %d", z->nxb, z->nvb, which);
  static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int64_t) == sizeof(double), "limbs are 64-bit words");
  CallBuf<long long> rows(c->mem);   // the limbs; the three counters of terms not summed lie behind them
  if (int rc = rows.take(n + 4, who, "the histogram's rows")) return rc;
  HIP_TRY(hipMemsetAsync(rows.p, 0, sizeof(long long) * (n + 4), c->st));
  ZoomArgs a{};
  a.acc = rows.p, a.rej = rows.p + n;
  a.inv_q_p = std::ldexp(1.0, -e[1]), a.inv_q_w = std::ldexp(1.0, -e[2]);
  const PSet &A = S.set[c->cur];
  auto pass = [&](int i) { return launch_zoom(A.x, A.v, S.p, A.w, S.np, zg, which, a, plan.pass[i], c->cfg.dyn_tail, c->st); };
  if (int rc = run_passes(c, kTagZoom, c->cnt.zoom_passes, plan.npass, S.np, pass)) return rc;
  int64_t rej[4] = {0, 0, 0, 0};
  if (int rc = words_to_host(c, rej, rows.p + n, 4)) return rc;   // (the wait: every pass has ended)
  for (int k = 0; k < 3; ++k) c->cnt.zoom_rejected += rej[k];
  for (int k = 0; k < 3; ++k)
    if (rej[k] != 0)
      return fail(PIC1DP_ERR_ARG,
                  "%s: %lld term(s) of species %d, plane %s, lay at or beyond 2^44 quanta of 2^%d or were NaN (|p| or |w| far past the "
                  "bounds the input gives) and were not summed; nothing was handed out",
                  who, static_cast<long long>(rej[k]), isp, kPlaneName[k], e[k]);
  if (int rc = words_to_host(c, limbs, rows.p, static_cast<int64_t>(n))) return rc;
  zoom_fx_normalise(limbs, zoom_planes(which), cells);
  return 0;
}

}  // namespace

extern "C" {

int pic1dp_hip_zoom_len(const pic1dp_zoom *z, int32_t which, int64_t *n) {
  if (!z || !n) return fail(PIC1DP_ERR_ARG, "zoom_len: null argument");
  if (which < 1 || which > 7) return fail(PIC1DP_ERR_ARG, "zoom_len: which = %d, must be a mask of 1 (markr), 2 (total) and 4 (pertb)", which);
  if (z->nxb < 1 || z->nvb < 1 || z->nxb > ZOOM_MAX_BINS || z->nvb > ZOOM_MAX_BINS || static_cast<int64_t>(z->nxb) * z->nvb > ZOOM_MAX_CELLS)
    return fail(PIC1DP_ERR_ARG, "zoom_len: %d x %d cells: nxb and nvb must lie in 1..4096 and nxb * nvb must not exceed 2^20", z->nxb, z->nvb);
  *n = static_cast<int64_t>(zoom_planes(which)) * z->nxb * z->nvb;
  return 0;
}

int pic1dp_hip_zoom_limbs_len(const pic1dp_zoom *z, int32_t which, int64_t *n) {
  int64_t m = 0;
  if (!z || !n) return fail(PIC1DP_ERR_ARG, "zoom_limbs_len: null argument");
  if (int rc = pic1dp_hip_zoom_len(z, which, &m)) return rc;
  *n = 2 * m;
  return 0;
}

int pic1dp_hip_zoom_local_exact(pic1dp_ctx *c, int32_t isp, const pic1dp_zoom *z, int32_t which, int64_t *limbs) {
  return zoom_local(c, "zoom_local_exact", isp, z, which, limbs);
}

int pic1dp_hip_zoom_convert(const pic1dp_input *in, int32_t isp, const pic1dp_zoom *z, int32_t which, const int64_t *limbs, double *out) {
  int32_t e[3];
  if (int rc = zoom_refusals("zoom_convert", in, isp, z, which, e)) return rc;
  if (!limbs || !out) return fail(PIC1DP_ERR_ARG, "zoom_convert: null array");
  zoom_fx_convert(e, which, limbs, static_cast<size_t>(z->nxb) * z->nvb, out);
  return 0;
}

int pic1dp_hip_zoom(pic1dp_ctx *c, int32_t isp, const pic1dp_zoom *z, int32_t which, double *out) {
  CHECK_CTX(c);
  int32_t e[3];
  if (int rc = zoom_refusals("zoom", &c->in, isp, z, which, e)) return rc;
  if (!out) return fail(PIC1DP_ERR_ARG, "zoom: null output");
  const size_t cells = static_cast<size_t>(z->nxb) * z->nvb;
  std::vector<int64_t> limbs(2 * cells * zoom_planes(which));
  if (int rc = zoom_local(c, "zoom", isp, z, which, limbs.data())) return rc;
  zoom_fx_convert(e, which, limbs.data(), cells, out);
  return 0;
}

int pic1dp_hip_host_zoom(const pic1dp_input *in, int32_t isp, const pic1dp_zoom *z, int32_t which, const double *x, const double *v,
                         const double *p, const double *w, int64_t np, int64_t *limbs, int64_t rejected[3]) {
  int32_t e[3];
  if (int rc = zoom_refusals("host_zoom", in, isp, z, which, e)) return rc;
  if (np < 0) return fail(PIC1DP_ERR_ARG, "host_zoom: np = %lld is negative", static_cast<long long>(np));
  if (!limbs || !rejected) return fail(PIC1DP_ERR_ARG, "host_zoom: null output");
  if (np > 0 && (!x || !v || ((which & 2) && !p) || ((which & 4) && !w))) return fail(PIC1DP_ERR_ARG, "host_zoom: null marker array");
  zoom_host_sums(zoom_geom(*z, in->lx), which, e[1], e[2], x, v, p, w, np, limbs, rejected);
  return 0;
}

}  // extern "C"
