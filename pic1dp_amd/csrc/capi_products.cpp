// capi_products.cpp -- the read-only marker products computed on demand behind the C ABI of include/pic1dp_hip.h: the velocity
// moments on the field grid (pic1dp_hip_moments), their exact kind (2.15), the wave-particle power on the
// output grid (2.17) and its exact kind (2.19).  Passes of their own that cache nothing and change nothing, all of one shape:
// refusals, product_begin, the plan, prod_buffers, run_passes, prod_fetch, the product's own arithmetic on the host (DESIGN.md 1:
// how to add one).
#include "ctx.hpp"
#include "moments_fx.hpp"
#include "power_fx.hpp"

namespace pic1dp_host {

int product_check(pic1dp_ctx *c, const char *who, int32_t isp) {
  if (isp < 0 || isp >= c->in.nspecies) return fail(PIC1DP_ERR_ARG, "%s: bad species index %d", who, isp);
  if (!c->loaded) return fail(PIC1DP_ERR_STATE, "no particles: call particle_load or particles_upload first");
  return 0;
}

int product_begin(pic1dp_ctx *c, const char *who, int32_t isp) {
  if (int rc = product_check(c, who, isp)) return rc;
  return call_site(c, Call::ReadMarkers);   // (as state_digest: a noted push becomes memory; clean: nothing is launched)
}

}  // namespace pic1dp_host

namespace {

// which weight sets: 1 p, 2 w, 3 both; no w in a full-f run (deltaf < 0: no input to say); noun: "planes" of the moments, "plane" of the power
int which_refusal(const char *who, int32_t which, int deltaf, const char *noun) {
  if (which < 1 || which > 3) return fail(PIC1DP_ERR_ARG, "%s: which = %d, must be 1 (weights p), 2 (weights w) or 3 (both)", who, which);
  if ((which & 2) && deltaf == 0)
    return fail(PIC1DP_ERR_ARG, "%s: which = %d asks for the %s of w (which & 2), but a full-f context (deltaf = 0) has no w", who, which, noun);
  return 0;
}

int power_refusal(const char *who, const pic1dp_input &in, int32_t which) {   // the power's refusals that need no context
  if (int rc = which_refusal(who, which, in.deltaf, "plane")) return rc;
  if (in.nx_opd < 1 || in.nv_opd < 2)
    return fail(PIC1DP_ERR_ARG, "%s: nx_opd = %d, nv_opd = %d: nx_opd >= 1 and nv_opd >= 2 required", who, in.nx_opd, in.nv_opd);
  return 0;
}

// `words` 8-byte words of the product buffer zeroed on the stream, and as many of pinned staging (*h); every product ends with a stream wait: neither is in use
int prod_buffers(pic1dp_ctx *c, size_t words, double **h) {
  if (c->d_prod_words < words) {
    c->d_prod_words = 0;
    HIP_TRY(c->mem.regrow(&c->d_prod, words));
    c->d_prod_words = words;
  }
  if (int rc = pinned(c, words, h)) return rc;
  HIP_TRY(hipMemsetAsync(c->d_prod, 0, sizeof(double) * words, c->st));
  return 0;
}

int prod_fetch(pic1dp_ctx *c, size_t words, double *h) {   // ... and what the passes left there on the host: one copy, one wait
  HIP_TRY(hipMemcpyAsync(h, c->d_prod, sizeof(double) * words, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  return 0;
}

// this context's exact sums of species isp, normalised, in the pinned staging (*limbs) [sets][4][2][nx]; terms not summed: counted, PIC1DP_ERR_ARG
int moments_exact_local(pic1dp_ctx *c, const char *who, int32_t isp, int32_t which, const void *out, int64_t **limbs) {
  CHECK_CTX(c);
  if (int rc = which_refusal(who, which, c->in.deltaf, "planes")) return rc;
  if (!out) return fail(PIC1DP_ERR_ARG, "%s: null output", who);
  if (int rc = product_begin(c, who, isp)) return rc;
  int32_t e[4];
  if (int rc = pic1dp_hip_moments_quanta(&c->in, isp, e)) return rc;
  const int nx = c->in.nx;
  const Species &S = c->sp[isp];
  const MomentsPlan plan = moments_plan_exact(nx, which, c->in.deltaf, S.np, c->num_cu);
  if (plan.npass < 1) return fail(PIC1DP_ERR_STATE, "internal: moments_plan_exact has no pass for nx %d, which %d", nx, which);
  const size_t n = static_cast<size_t>(plan.selected) * 2 * nx;   // the limbs; the 8 counters of terms not summed lie behind them
  double *h = nullptr;
  if (int rc = prod_buffers(c, n + 8, &h)) return rc;
  static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int64_t) == sizeof(double), "limbs are 64-bit words");
  MomentsFxArgs a{};
  a.acc = reinterpret_cast<long long *>(c->d_prod), a.rej = a.acc + n;
  for (int k = 0; k < 4; ++k) a.inv_q[k] = std::ldexp(1.0, -e[k]);
  const PSet &A = S.set[c->cur];
  auto pass = [&](int i) { return launch_moments_exact(A.x, A.v, S.p, A.w, S.np, c->grid, a, plan.pass[i], c->cfg.dyn_tail, c->st); };
  if (int rc = run_passes(c, kTagMomentsExact, c->cnt.moments_exact_passes, plan.npass, S.np, pass)) return rc;
  if (int rc = prod_fetch(c, n + 8, h)) return rc;
  *limbs = reinterpret_cast<int64_t *>(h);
  const int64_t *rej = *limbs + n;
  int first = -1;
  for (int j = 0; j < plan.selected; ++j) {
    c->cnt.moments_exact_rejected += rej[j];
    if (rej[j] != 0 && first < 0) first = j;
  }
  if (first >= 0) {
    const bool is_w = which == 2 || first >= 4;
    return fail(PIC1DP_ERR_ARG,
                "%s: %lld term(s) of species %d, weight set %s, power v^%d, lay at or beyond 2^44 quanta of 2^%d or were NaN (|p|, |w| "
                "or |v| far past the bounds the input gives) and were not summed; nothing was handed out",
                who, static_cast<long long>(rej[first]), isp, is_w ? "w" : "p", first & 3, e[first & 3]);
  }
  moments_fx_normalise(*limbs, plan.selected, nx);
  return 0;
}

// e_base = kb + kvm - 40 of a species, from the input alone
int power_exact_base(const char *who, const pic1dp_input &in, int32_t isp, int32_t *e_base) {
  int32_t cq = 0;
  if (int rc = pic1dp_hip_charge_quantum(&in, isp, &cq)) return rc;   // (the input's version and species index with it)
  if (!power_fx_base(cq, in.v_max, e_base)) return fail(PIC1DP_ERR_ARG, "%s: v_max must be positive and finite", who);
  return 0;
}

// this context's exact power sums of species isp, normalised, in the pinned staging (*limbs) [sets][2 nxv + 2], and the call's e;
// a field that is not finite, terms not summed: PIC1DP_ERR_ARG
int power_exact_local(pic1dp_ctx *c, const char *who, int32_t isp, int32_t which, const void *out, int64_t **limbs, int32_t *e) {
  CHECK_CTX(c);
  const pic1dp_input &in = c->in;
  if (int rc = power_refusal(who, in, which)) return rc;
  if (!out || !e) return fail(PIC1DP_ERR_ARG, "%s: null output", who);
  if (isp < 0 || isp >= in.nspecies) return fail(PIC1DP_ERR_ARG, "%s: bad species index %d", who, isp);
  int32_t e_base = 0;
  if (int rc = power_exact_base(who, in, isp, &e_base)) return rc;
  if (int rc = product_begin(c, who, isp)) return rc;
  if (int rc = call_site(c, Call::ReadField)) return rc;    // (as pic1dp_hip_get_field: d_E is field_electric)
  const Species &S = c->sp[isp];
  const PowerPlan plan = power_plan_exact(in.nx, in.nx_opd, in.nv_opd, which, in.deltaf, S.np, c->num_cu);
  if (plan.npass < 1) return fail(PIC1DP_ERR_STATE, "internal: power_plan_exact has no pass for nx %d, %d x %d, which %d", in.nx, in.nx_opd, in.nv_opd, which);
  const size_t nsets = static_cast<size_t>(plan.selected), n = nsets * power_fx_set_words(in.nx_opd, in.nv_opd);
  // behind the limbs: [4] terms not summed (per set: bins, rest), [3] e, the non-finite flag, the bits of max |E|, [1]
  // padding; a species without markers launches nothing: the field itself travels in their place
  const size_t nx = static_cast<size_t>(in.nx), words = n + 8 + (S.np > 0 ? 0 : nx);
  double *h = nullptr;
  if (int rc = prod_buffers(c, words, &h)) return rc;
  static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int64_t) == sizeof(double), "limbs are 64-bit words");
  PowerFxArgs a{};
  a.acc = reinterpret_cast<long long *>(c->d_prod), a.rej = a.acc + n, a.scale = a.rej + 4, a.e_base = e_base;
  const PSet &A = S.set[c->cur];
  auto pass = [&](int i) {
    return launch_power_exact(A.x, A.v, S.p, A.w, S.np, c->grid, dist_geom(c), c->d_E, a, plan.pass[i], c->cfg.dyn_tail, c->st);
  };
  int64_t launched = 0;   // (counted once the field is known to be finite: other passes sweep no marker)
  if (int rc = run_passes(c, kTagPowerExact, launched, plan.npass, S.np, pass)) return rc;
  if (S.np <= 0) HIP_TRY(hipMemcpyAsync(c->d_prod + n + 8, c->d_E, sizeof(double) * nx, hipMemcpyDeviceToDevice, c->st));
  if (int rc = prod_fetch(c, words, h)) return rc;
  if (int rc = xchg_check(c)) return rc;
  *limbs = reinterpret_cast<int64_t *>(h);
  const int64_t *rej = *limbs + n, *scale = rej + 4;
  bool finite = scale[1] == 0;
  int32_t e_call = static_cast<int32_t>(scale[0]);
  if (S.np <= 0) {   // the device's rule on the host (power_fx_quantum: the two agree at every double)
    double mx = 0.0;
    for (size_t i = 0; i < nx && finite; ++i) {
      finite = std::isfinite(h[n + 8 + i]);
      mx = std::fmax(mx, std::fabs(h[n + 8 + i]));
    }
    if (finite) power_fx_quantum(e_base, mx, &e_call);
  }
  if (!finite) return fail(PIC1DP_ERR_ARG, "%s: field not finite: field_electric holds an infinity or a NaN; no marker was read, nothing was handed out", who);
  c->cnt.power_exact_passes += launched;
  for (size_t j = 0; j < nsets; ++j) c->cnt.power_exact_rejected += rej[2 * j] + rej[2 * j + 1];
  for (size_t j = 0; j < 2 * nsets; ++j)
    if (rej[j] != 0) {
      const bool is_w = which == 2 || j >= 2;
      return fail(PIC1DP_ERR_ARG,
                  "%s: %lld term(s) of species %d, weight set %s, %s, lay at or beyond 2^44 quanta of 2^%d or were NaN (|p|, |w| or |v| "
                  "far past the bounds the input gives) and were not summed; nothing was handed out",
                  who, static_cast<long long>(rej[j]), isp, is_w ? "w" : "p", (j & 1) ? "rest" : "bins", e_call);
    }
  power_fx_normalise(*limbs, plan.selected, in.nx_opd, in.nv_opd);
  *e = e_call;
  return 0;
}

}  // namespace

extern "C" {

// ---- velocity moments of the markers on the field grid ----
int pic1dp_hip_moments(pic1dp_ctx *c, int32_t isp, int32_t which, double *out) {
  CHECK_CTX(c);
  if (int rc = which_refusal("moments", which, c->in.deltaf, "planes")) return rc;
  if (!out) return fail(PIC1DP_ERR_ARG, "moments: null output");
  if (int rc = product_begin(c, "moments", isp)) return rc;
  const int nx = c->in.nx;
  const Species &S = c->sp[isp];
  const MomentsPlan plan = moments_plan(nx, which, c->in.deltaf, S.np, c->num_cu);
  if (plan.npass < 1) return fail(PIC1DP_ERR_STATE, "internal: moments_plan has no pass for nx %d, which %d", nx, which);
  const size_t n = static_cast<size_t>(plan.selected) * nx;
  double *h = nullptr;
  if (int rc = prod_buffers(c, n, &h)) return rc;
  const PSet &A = S.set[c->cur];
  auto pass = [&](int i) { return launch_moments(A.x, A.v, S.p, A.w, S.np, c->grid, c->d_prod, plan.pass[i], c->cfg.dyn_tail, c->st); };
  if (int rc = run_passes(c, kTagMoments, c->cnt.moments_passes, plan.npass, S.np, pass)) return rc;
  if (int rc = prod_fetch(c, n, h)) return rc;
  std::memcpy(out, h, sizeof(double) * n);
  return 0;
}

// ---- velocity-resolved wave-particle power on the output grid ----
int pic1dp_hip_power_len(const pic1dp_input *in, int32_t which, int64_t *n) {
  if (!in || !n) return fail(PIC1DP_ERR_ARG, "power_len: null argument");
  if (int rc = power_refusal("power_len", *in, which)) return rc;
  const int64_t nxv = static_cast<int64_t>(in->nx_opd) * in->nv_opd;
  *n = (which == 3 ? 2 : 1) * (nxv + in->nv_opd + 1);
  return 0;
}

int pic1dp_hip_power(pic1dp_ctx *c, int32_t isp, int32_t which, double *out) {
  CHECK_CTX(c);
  const pic1dp_input &in = c->in;
  if (int rc = power_refusal("power", in, which)) return rc;
  if (!out) return fail(PIC1DP_ERR_ARG, "power: null output");
  if (int rc = product_begin(c, "power", isp)) return rc;
  if (int rc = call_site(c, Call::ReadField)) return rc;    // (as pic1dp_hip_get_field: d_E is field_electric)
  const Species &S = c->sp[isp];
  const PowerPlan plan = power_plan(in.nx, in.nx_opd, in.nv_opd, which, in.deltaf, S.np, c->num_cu);
  if (plan.npass < 1) return fail(PIC1DP_ERR_STATE, "internal: power_plan has no pass for nx %d, %d x %d, which %d", in.nx, in.nx_opd, in.nv_opd, which);
  const size_t nxv = static_cast<size_t>(in.nx_opd) * in.nv_opd, nvo = static_cast<size_t>(in.nv_opd);
  const size_t nsets = static_cast<size_t>(plan.selected), n = nsets * nxv + nsets;   // the planes, then a rest word per set
  double *h = nullptr;
  if (int rc = prod_buffers(c, n, &h)) return rc;
  double *d_rest = c->d_prod + nsets * nxv;
  const PSet &A = S.set[c->cur];
  auto pass = [&](int i) {
    return launch_power(A.x, A.v, S.p, A.w, S.np, c->grid, dist_geom(c), c->d_E, c->d_prod, d_rest, plan.pass[i], c->cfg.dyn_tail, c->st);
  };
  if (int rc = run_passes(c, kTagPower, c->cnt.power_passes, plan.npass, S.np, pass)) return rc;
  if (int rc = prod_fetch(c, n, h)) return rc;
  if (int rc = xchg_check(c)) return rc;
  // per set: [plane | v-profile = the plane summed over ix ascending | rest]
  for (size_t j = 0; j < nsets; ++j) {
    const double *plane = h + j * nxv;
    double *o = out + j * (nxv + nvo + 1);
    std::memcpy(o, plane, sizeof(double) * nxv);
    for (size_t iv = 0; iv < nvo; ++iv) {
      double acc = 0.0;
      for (int ix = 0; ix < in.nx_opd; ++ix) acc += plane[iv * in.nx_opd + ix];
      o[nxv + iv] = acc;
    }
    o[nxv + nvo] = h[nsets * nxv + j];
  }
  return 0;
}

// ---- the exact kind of the power: the same terms in whole quanta 2^e, e from max |E| of the call (the arithmetic on the host: power_fx.cpp) ----
int pic1dp_hip_power_quantum(const pic1dp_input *in, int32_t isp, double max_abs_E, int32_t *e) {
  if (!in || !e) return fail(PIC1DP_ERR_ARG, "power_quantum: null argument");
  int32_t e_base = 0;
  if (int rc = power_exact_base("power_quantum", *in, isp, &e_base)) return rc;
  if (!power_fx_quantum(e_base, max_abs_E, e)) return fail(PIC1DP_ERR_ARG, "power_quantum: field not finite: max_abs_E must be finite and not negative");
  return 0;
}

int pic1dp_hip_power_limbs_len(const pic1dp_input *in, int32_t which, int64_t *n) {
  if (!in || !n) return fail(PIC1DP_ERR_ARG, "power_limbs_len: null argument");
  if (int rc = power_refusal("power_limbs_len", *in, which)) return rc;
  *n = static_cast<int64_t>(which == 3 ? 2 : 1) * static_cast<int64_t>(power_fx_set_words(in->nx_opd, in->nv_opd));
  return 0;
}

int pic1dp_hip_power_local_exact(pic1dp_ctx *c, int32_t isp, int32_t which, int64_t *limbs, int32_t *e) {
  int64_t *h = nullptr;
  int32_t e_call = 0;
  if (int rc = power_exact_local(c, "power_local_exact", isp, which, limbs, &h, e ? &e_call : nullptr)) return rc;
  std::memcpy(limbs, h, sizeof(int64_t) * (which == 3 ? 2 : 1) * power_fx_set_words(c->in.nx_opd, c->in.nv_opd));
  *e = e_call;
  return 0;
}

int pic1dp_hip_power_convert(const pic1dp_input *in, int32_t which, int32_t e, const int64_t *limbs, double *out) {
  if (!in) return fail(PIC1DP_ERR_ARG, "power_convert: null input");
  if (int rc = power_refusal("power_convert", *in, which)) return rc;
  if (!limbs || !out) return fail(PIC1DP_ERR_ARG, "power_convert: null array");
  power_fx_convert(e, limbs, which == 3 ? 2 : 1, in->nx_opd, in->nv_opd, out);
  return 0;
}

int pic1dp_hip_power_exact(pic1dp_ctx *c, int32_t isp, int32_t which, double *out) {
  int64_t *h = nullptr;
  int32_t e = 0;
  if (int rc = power_exact_local(c, "power_exact", isp, which, out, &h, &e)) return rc;
  power_fx_convert(e, h, which == 3 ? 2 : 1, c->in.nx_opd, c->in.nv_opd, out);
  return 0;
}

// ---- the exact kind of the moments: the same terms in whole quanta, integer sums (the arithmetic on the host: moments_fx.cpp) ----
int pic1dp_hip_moments_quanta(const pic1dp_input *in, int32_t isp, int32_t e[4]) {
  if (!in || !e) return fail(PIC1DP_ERR_ARG, "moments_quanta: null argument");
  int32_t cq = 0;
  if (int rc = pic1dp_hip_charge_quantum(in, isp, &cq)) return rc;
  if (!moments_fx_quanta(cq, in->v_max, e)) return fail(PIC1DP_ERR_ARG, "moments_quanta: v_max must be positive and finite");
  return 0;
}

int pic1dp_hip_moments_limbs_len(int32_t which, int32_t nx, int64_t *n) {
  if (!n) return fail(PIC1DP_ERR_ARG, "moments_limbs_len: null argument");
  if (int rc = which_refusal("moments_limbs_len", which, -1, "planes")) return rc;
  if (nx < 1) return fail(PIC1DP_ERR_ARG, "moments_limbs_len: nx = %d", nx);
  *n = static_cast<int64_t>(which == 3 ? 16 : 8) * nx;
  return 0;
}

int pic1dp_hip_moments_local_exact(pic1dp_ctx *c, int32_t isp, int32_t which, int64_t *limbs) {
  int64_t *h = nullptr;
  if (int rc = moments_exact_local(c, "moments_local_exact", isp, which, limbs, &h)) return rc;
  std::memcpy(limbs, h, sizeof(int64_t) * static_cast<size_t>(which == 3 ? 16 : 8) * c->in.nx);
  return 0;
}

int pic1dp_hip_moments_convert(const pic1dp_input *in, int32_t isp, int32_t which, const int64_t *limbs, double *out) {
  if (!in) return fail(PIC1DP_ERR_ARG, "moments_convert: null input");
  int32_t e[4];
  if (int rc = pic1dp_hip_moments_quanta(in, isp, e)) return rc;   // (the input's version and species index with it)
  if (int rc = which_refusal("moments_convert", which, in->deltaf, "planes")) return rc;
  if (!limbs || !out) return fail(PIC1DP_ERR_ARG, "moments_convert: null array");
  if (in->nx < 1) return fail(PIC1DP_ERR_ARG, "moments_convert: nx = %d", in->nx);
  moments_fx_convert(e, limbs, which == 3 ? 8 : 4, in->nx, out);
  return 0;
}

int pic1dp_hip_moments_exact(pic1dp_ctx *c, int32_t isp, int32_t which, double *out) {
  int64_t *h = nullptr;
  if (int rc = moments_exact_local(c, "moments_exact", isp, which, out, &h)) return rc;
  int32_t e[4];
  if (int rc = pic1dp_hip_moments_quanta(&c->in, isp, e)) return rc;
  moments_fx_convert(e, h, which == 3 ? 8 : 4, c->in.nx, out);
  return 0;
}

}  // extern "C"
