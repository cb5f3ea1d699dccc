// capi_hermite.cpp -- the Fourier-Hermite spectrum of a species' markers behind the C ABI (include/pic1dp_hip.h
// pic1dp_hip_hermite, _hermite_len, _host_hermite, _hermite_tables): one pass of its own in the
// mould of capi_products.cpp, which caches nothing and changes nothing.  The tables and the device words are the context's
// from the first call on (DeviceMem); the words cross to the host through the pinned staging in one copy.  The entry points
// that take no context make no HIP call.
#include "ctx.hpp"
#include "select_rule.hpp"

namespace {

constexpr size_t kTabWords = 2 * HERM_MAX_N, kAccWords = static_cast<size_t>(HERM_MAX_N) * HERM_MAX_COLS;

// the refusals that need no input: null, which, the sizes, the modes among themselves, v0 and vt
int hermite_shape_refusal(const char *who, const pic1dp_hermite *h, int32_t which) {
  if (!h) return fail(PIC1DP_ERR_ARG, "%s: null spectrum description", who);
  if (which < 1 || which > 3) return fail(PIC1DP_ERR_ARG, "%s: which = %d, must be 1 (weights p), 2 (weights w) or 3 (both)", who, which);
  if (h->nherm < 1 || h->nherm > HERM_MAX_N) return fail(PIC1DP_ERR_ARG, "%s: nherm = %d, must lie in 1..%d", who, h->nherm, HERM_MAX_N);
  const int sets = which == 3 ? 2 : 1;
  if (h->nmodes < 1 || sets * h->nmodes > HERM_MAX_MODES)
    return fail(PIC1DP_ERR_ARG, "%s: nmodes = %d with %d weight set(s): 1 <= nmodes and sets * nmodes <= %d required", who, h->nmodes, sets,
                HERM_MAX_MODES);
  for (int a = 0; a < h->nmodes; ++a) {
    if (h->modes[a] < 0) return fail(PIC1DP_ERR_ARG, "%s: mode %d is negative", who, h->modes[a]);
    for (int b = 0; b < a; ++b)
      if (h->modes[a] == h->modes[b]) return fail(PIC1DP_ERR_ARG, "%s: mode %d is listed twice", who, h->modes[a]);
  }
  if (!std::isfinite(h->v0) || !std::isfinite(h->vt) || !(h->vt > 0.0))
    return fail(PIC1DP_ERR_ARG, "%s: v0 = %g, vt = %g: v0 finite and vt finite and positive required", who, h->v0, h->vt);
  return 0;
}

// ... and those that need the input: w of a full-f run, the modes against the grid, the species
int hermite_refusal(const char *who, const pic1dp_input *in, int32_t isp, int32_t which, const pic1dp_hermite *h) {
  if (!in) return fail(PIC1DP_ERR_ARG, "%s: null input", who);
  if (int rc = hermite_shape_refusal(who, h, which)) return rc;
  if ((which & 2) && in->deltaf == 0)
    return fail(PIC1DP_ERR_ARG, "%s: which = %d asks for the spectrum of w (which & 2), but a full-f context (deltaf = 0) has no w", who, which);
  for (int a = 0; a < h->nmodes; ++a)
    if (h->modes[a] > in->nx / 2) return fail(PIC1DP_ERR_ARG, "%s: mode %d lies beyond nx / 2 = %d", who, h->modes[a], in->nx / 2);
  if (isp < 0 || isp >= in->nspecies) return fail(PIC1DP_ERR_ARG, "%s: bad species index %d", who, isp);
  return 0;
}

// kk[a] = 2 pi / lx * m: loader.cpp's expression for the init modes
void hermite_wavenumbers(const pic1dp_input &in, const pic1dp_hermite &h, double kk[HERM_MAX_MODES]) {
  for (int a = 0; a < HERM_MAX_MODES; ++a) kk[a] = a < h.nmodes ? 2.0 * kPi / in.lx * static_cast<double>(h.modes[a]) : 0.0;
}

// the tables and the words on the device, the context's from the first call on
int hermite_device(pic1dp_ctx *c) {
  if (c->d_herm) return 0;
  const hipError_t e = c->mem.alloc(&c->d_herm, kTabWords + kAccWords);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    c->d_herm = nullptr;
    return fail(e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation ? PIC1DP_ERR_NOMEM : PIC1DP_ERR_HIP,
                "hermite: allocating the tables and words failed: %s", hipGetErrorString(e));
  }
  double tab[kTabWords];
  hermite_tables_host(HERM_MAX_N, tab, tab + HERM_MAX_N);
  const hipError_t up = hipMemcpy(c->d_herm, tab, sizeof tab, hipMemcpyHostToDevice);
  if (up != hipSuccess) {   // (no buffer without its tables: the next call starts over)
    c->mem.release(&c->d_herm);
    return fail(PIC1DP_ERR_HIP, "hermite: uploading the tables failed: %s", hipGetErrorString(up));
  }
  return 0;
}

}  // namespace

extern "C" {

int pic1dp_hip_hermite_len(const pic1dp_hermite *h, int32_t which, int64_t *n) {
  if (!n) return fail(PIC1DP_ERR_ARG, "hermite_len: null argument");
  if (int rc = hermite_shape_refusal("hermite_len", h, which)) return rc;
  *n = static_cast<int64_t>(which == 3 ? 2 : 1) * h->nmodes * 2 * h->nherm;
  return 0;
}

int pic1dp_hip_hermite_tables(int32_t nherm, double *ra, double *rb) {
  if (!ra || !rb) return fail(PIC1DP_ERR_ARG, "hermite_tables: null array");
  if (nherm < 1 || nherm > HERM_MAX_N) return fail(PIC1DP_ERR_ARG, "hermite_tables: nherm = %d, must lie in 1..%d", nherm, HERM_MAX_N);
  hermite_tables_host(nherm, ra, rb);
  return 0;
}

int pic1dp_hip_host_hermite(const pic1dp_input *in, int32_t isp, int32_t which, const pic1dp_hermite *h, int64_t np, const double *x,
                            const double *v, const double *p, const double *w, double *out) {
  if (int rc = hermite_refusal("host_hermite", in, isp, which, h)) return rc;
  if (np < 0) return fail(PIC1DP_ERR_ARG, "host_hermite: np = %lld is negative", static_cast<long long>(np));
  if (!out) return fail(PIC1DP_ERR_ARG, "host_hermite: null output");
  if (np > 0 && (!x || !v || ((which & 1) && !p) || ((which & 2) && !w))) return fail(PIC1DP_ERR_ARG, "host_hermite: null marker array");
  const int nh = h->nherm, nm = h->nmodes, sets = which == 3 ? 2 : 1;
  double ra[HERM_MAX_N], rb[HERM_MAX_N], kk[HERM_MAX_MODES], psi[HERM_MAX_N];
  hermite_tables_host(nh, ra, rb);
  hermite_wavenumbers(*in, *h, kk);
  const double ivt = 1.0 / h->vt;
  std::fill(out, out + static_cast<size_t>(sets) * nm * 2 * nh, 0.0);
  for (int64_t i = 0; i < np; ++i) {
    const double px = select_wrap(x[i], in->lx);
    const double u = (v[i] - h->v0) * ivt;
    double prev = 0.0, cur = 1.0;
    for (int n = 0; n < nh; ++n) {
      psi[n] = cur;
      double nx = u;
      if (n > 0) {
        const double a = u * cur;
        nx = a * ra[n] - prev * rb[n];
      }
      prev = cur, cur = nx;
    }
    for (int a = 0; a < nm; ++a) {
      double sn, cs;
      ::sincos(kk[a] * px, &sn, &cs);
      for (int j = 0; j < sets; ++j) {
        const double q = (which == 2 || j == 1) ? w[i] : p[i];
        const double yc = q * cs, ys = q * sn;
        double *oc = out + (static_cast<size_t>(j) * nm + a) * 2 * nh, *os = oc + nh;
        for (int n = 0; n < nh; ++n) {
          oc[n] = oc[n] + psi[n] * yc;
          os[n] = os[n] + psi[n] * ys;
        }
      }
    }
  }
  return 0;
}

int pic1dp_hip_hermite(pic1dp_ctx *c, int32_t isp, int32_t which, const pic1dp_hermite *h, double *out) {
  CHECK_CTX(c);
  if (int rc = hermite_refusal("hermite", &c->in, isp, which, h)) return rc;
  if (!out) return fail(PIC1DP_ERR_ARG, "hermite: null output");
  if (int rc = product_begin(c, "hermite", isp)) return rc;
  const Species &S = c->sp[isp];
  const int nh = h->nherm, nm = h->nmodes, sets = which == 3 ? 2 : 1;
  const HermitePlan plan = hermite_plan(nh, nm, which, c->in.deltaf, S.np, c->num_cu);
  if (plan.blocks < 1) return fail(PIC1DP_ERR_STATE, "internal: hermite_plan has no pass for nherm %d, %d modes, which %d", nh, nm, which);
  if (int rc = hermite_device(c)) return rc;
  const size_t words = static_cast<size_t>(plan.nb) * 16 * HERM_MAX_COLS;
  double *hp = nullptr;
  if (int rc = pinned(c, words, &hp)) return rc;
  HermiteArgs a{};
  a.tab = c->d_herm, a.acc = c->d_herm + kTabWords;
  a.v0 = h->v0, a.ivt = 1.0 / h->vt, a.lx = c->in.lx;
  hermite_wavenumbers(c->in, *h, a.kk);
  a.nmodes = nm, a.nherm = nh;
  HIP_TRY(hipMemsetAsync(a.acc, 0, sizeof(double) * words, c->st));
  const PSet &A = S.set[c->cur];
  auto pass = [&](int) { return launch_hermite(A.x, A.v, S.p, A.w, S.np, (which & 1) != 0, (which & 2) != 0, a, plan, c->st); };
  if (int rc = run_passes(c, kTagHermite, c->cnt.hermite_passes, 1, S.np, pass)) return rc;
  HIP_TRY(hipMemcpyAsync(hp, a.acc, sizeof(double) * words, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  // the device's [n][column] to the caller's [column][n]: rows from nherm on and columns beyond the selected ones stay behind
  const int ncol = sets * nm * 2;
  for (int col = 0; col < ncol; ++col)
    for (int n = 0; n < nh; ++n) out[static_cast<size_t>(col) * nh + n] = hp[static_cast<size_t>(n) * HERM_MAX_COLS + col];
  return 0;
}

}  // extern "C"
