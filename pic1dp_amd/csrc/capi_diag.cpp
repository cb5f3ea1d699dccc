// capi_diag.cpp -- diagnostics of output_all (src/pic1dp_output.F90:100-189, 196-477): the kinetic sums and the
// (x, v) / v histograms, one fused pass per species, cached against state_version; the FP64 kind and the exact kind
// (pic1dp_hip_set_diag_sum).  The products computed on demand, which cache nothing: capi_products.cpp.
#include "ctx.hpp"
#include "fx_limbs.hpp"

namespace pic1dp_host {

// One fused pass over a species' markers for output_all: histograms of
// output_ptcldist into d_dist[isp] and the kinetic sums of output_field; results
// stay valid until the markers change (state_version).
size_t dist_len(const pic1dp_input &in) {
  return 3 * static_cast<size_t>(in.nx_opd) * in.nv_opd + 3 * static_cast<size_t>(in.nv_opd);
}

int diag_max_blocks(const pic1dp_ctx *c) { return 2 * c->num_cu; }

int pinned(pic1dp_ctx *c, size_t ndoubles, double **out) {
  if (ndoubles > c->h_pin_doubles) {
    HIP_TRY(hipStreamSynchronize(c->st));  // (nothing in flight into the old buffer)
    c->h_pin_doubles = 0;
    const size_t want = ndoubles + ndoubles / 4 + 64;
    HIP_TRY(c->mem.regrow(&c->h_pin, want, true));
    c->h_pin_doubles = want;
  }
  *out = c->h_pin;
  return 0;
}

// the histogram geometry with its constant divisors vouched for, formed once per context
const DistGeom &dist_geom(pic1dp_ctx *c) {
  if (!c->dist_geom_ready) {
    c->dist_geom_v = make_dist_geom(c->in.lx, c->in.v_max, c->in.nx_opd, c->in.nv_opd);
    c->dist_geom_ready = true;
  }
  return c->dist_geom_v;
}

// buffers of the marker diagnostics: [nspecies] cached histograms + one for the all-reduced
// copy handed out, per-workgroup partial sums per species
int diag_buffers(pic1dp_ctx *c) {
  const pic1dp_input &in = c->in;
  const int ns = in.nspecies;
  if (in.nx_opd < 1 || in.nv_opd < 2) return fail(PIC1DP_ERR_ARG, "nx_opd >= 1 and nv_opd >= 2 required");
  if (!c->d_dist) HIP_TRY(c->mem.alloc(&c->d_dist, dist_len(in) * (ns + 1)));
  if (!c->d_diag_part) HIP_TRY(c->mem.alloc(&c->d_diag_part, static_cast<size_t>(DIAG_PART) * diag_max_blocks(c) * ns));
  return 0;
}

double *diag_part_dev(const pic1dp_ctx *c, int isp) { return c->d_diag_part + static_cast<size_t>(DIAG_PART) * diag_max_blocks(c) * isp; }

void diag_void_bounds(pic1dp_ctx *c) {
  for (DiagSpecies &D : c->diag) D.max_p = D.max_w = 0.0;
}

// may species isp's next pass sum its histograms in fixed point (device_diag.hpp DistScale), and within which bounds: its
// max |p|, max |w| of the pass before with a margin (p changes with load / upload / events only, w by a few per cent a record)
bool diag_fx_bounds(const pic1dp_ctx *c, int isp, double *bound_p, double *bound_w) {
  const DiagSpecies &D = c->diag[isp];
  if (!(c->cfg.diag_fx && D.max_p > 0.0 && (c->in.deltaf != 1 || D.max_w > 0.0))) return false;
  *bound_p = 2.0 * D.max_p;
  *bound_w = c->cfg.diag_fx_margin_w * D.max_w;
  return true;
}

// a pass over species isp's markers as they are now is enqueued: what the collector has to know, and the counters
// (launched: in a launch of its own, k_ptcldist or k_ptcldist_exact -- not k_step_full<DIAG>)
void diag_note_pass(pic1dp_ctx *c, int isp, int blocks, bool fixed, bool launched) {
  DiagSpecies &D = c->diag[isp];
  D.blocks = blocks, D.fixed = fixed, D.pending = true, D.version = c->state_version;
  if (launched) c->cnt.diag_passes++;
  if (fixed) c->cnt.diag_fx_passes++;
}

// the diagnostics' own pass over species isp (k_ptcldist) into its cached histograms; fixed: 64-bit fixed-point sums where
// diag_fx_bounds allows them, else -- and whenever `fixed` is false -- double sums
static int run_diag_pass(pic1dp_ctx *c, int isp, bool fixed) {
  const pic1dp_input &in = c->in;
  Species &S = c->sp[isp];
  const PSet &A = S.set[c->cur];
  const size_t ntot = dist_len(in);
  double *hist = c->d_dist + ntot * isp;
  HIP_TRY(hipMemsetAsync(hist, 0, sizeof(double) * ntot, c->st));
  int blocks = 0;
  bool was_fixed = false;
  if (S.np > 0) {
    double bp = 0.0, bw = 0.0;
    if (fixed) (void)diag_fx_bounds(c, isp, &bp, &bw);
    const DiagLaunch dl = diag_launch(0, S.np, in.nx_opd, in.nv_opd, c->num_cu);
    blocks = dl.blocks;
    HIP_TRY(launch_ptcldist(A.x, A.v, S.p, A.w, S.np, dist_geom(c), in.deltaf == 1, bp, bw, hist, diag_part_dev(c, isp), dl, c->cfg.dyn_tail,
                            c->st, &was_fixed));
  }
  diag_note_pass(c, isp, blocks, was_fixed, S.np > 0);
  return 0;
}

// a pass of kind 0 if nothing has seen these markers yet
static int diag_refresh(pic1dp_ctx *c, int isp) {
  return c->diag[isp].version == c->state_version ? 0 : run_diag_pass(c, isp, true);
}

// Where a species' results lie in the pinned staging: the pass's partial sums [diag_max_blocks][DIAG_PART], the tail
// slots' [kEnergyBlocks][3], the histograms [dist_len] (output_all only)
struct DiagSlots {
  double *part, *tail, *hist;
  static size_t len(const pic1dp_ctx *c, bool with_hist) {
    return static_cast<size_t>(DIAG_PART) * diag_max_blocks(c) + 3 * static_cast<size_t>(kEnergyBlocks) + (with_hist ? dist_len(c->in) : 0);
  }
  DiagSlots(const pic1dp_ctx *c, double *base)
      : part(base), tail(part + static_cast<size_t>(DIAG_PART) * diag_max_blocks(c)), hist(tail + 3 * static_cast<size_t>(kEnergyBlocks)) {}
};

// workgroups that sum the tail slots of species isp's pending pass (the reference sums the whole local vector, VecSum;
// slots beyond np live in set 0)
static int diag_tail_blocks(const pic1dp_ctx *c, int isp) {
  return c->diag[isp].pending ? tail_sum_blocks(c->sp[isp].nalloc - c->sp[isp].np) : 0;
}
// ... enqueued: their partial sums through d_scratch into the species' slot
static int enqueue_tail_sums(pic1dp_ctx *c, int isp, const DiagSlots &to) {
  const Species &S = c->sp[isp];
  const int tb = diag_tail_blocks(c, isp);
  if (tb == 0) return 0;
  HIP_TRY(launch_energy_sums(S.set[0].v, S.p, c->in.deltaf ? S.set[0].w : nullptr, S.np, S.nalloc - S.np, c->d_scratch, tb, c->st));
  HIP_TRY(hipMemcpyAsync(to.tail, c->d_scratch, sizeof(double) * tb * 3, hipMemcpyDeviceToHost, c->st));
  return 0;
}

// The collector: species isp's pending pass (its own, or k_step_full<DIAG> inside a step) from its slots, once they have
// arrived: the kinetic sums in workgroup order, then the tail slots'; the maxima the next pass may scale with.  A
// fixed-point pass skipped every marker beyond its bounds: the species once more in doubles (rare), into THIS species'
// slots only -- the rest of the buffer may still be unread --; the tail sums are the ones already there.
static int diag_collect(pic1dp_ctx *c, int isp, const DiagSlots &at, bool with_hist) {
  DiagSpecies &D = c->diag[isp];
  if (!D.pending) return 0;
  const int tb = diag_tail_blocks(c, isp);
  for (;;) {
    D.sums[0] = D.sums[1] = D.sums[2] = 0.0;
    double maxp = 0.0, maxw = 0.0, over = 0.0;
    for (int b = 0; b < D.blocks; ++b) {
      const double *q = at.part + static_cast<size_t>(b) * DIAG_PART;
      for (int k = 0; k < 3; ++k) D.sums[k] += q[k];
      maxp = std::max(maxp, q[3]);
      maxw = std::max(maxw, q[4]);
      over = std::max(over, q[5]);
    }
    for (int b = 0; b < tb; ++b)
      for (int k = 0; k < 3; ++k) D.sums[k] += at.tail[b * 3 + k];
    if (D.blocks > 0) D.max_p = maxp, D.max_w = maxw;
    if (!(D.fixed && over > 0.0)) break;
    c->cnt.diag_fx_repeats++;   // (the repeat is no fixed-point pass: the next round ends the loop)
    if (int rc = run_diag_pass(c, isp, false)) return rc;
    if (D.blocks > diag_max_blocks(c)) return fail(PIC1DP_ERR_STATE, "diagnostics: more partial sums than their slot holds");
    if (D.blocks > 0)
      HIP_TRY(hipMemcpyAsync(at.part, diag_part_dev(c, isp), sizeof(double) * DIAG_PART * D.blocks, hipMemcpyDeviceToHost, c->st));
    if (with_hist)
      HIP_TRY(hipMemcpyAsync(at.hist, c->d_dist + dist_len(c->in) * isp, sizeof(double) * dist_len(c->in), hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
  }
  D.pending = false;
  return 0;
}

// species isp's kinetic sums (DiagSpecies::sums) and cached histograms (d_dist) belong to the markers as they are: both
// transfers through the pinned staging enqueued, ONE wait
int ensure_diag(pic1dp_ctx *c, int isp) {
  if (int rc = diag_buffers(c)) return rc;
  if (int rc = diag_refresh(c, isp)) return rc;
  const DiagSpecies &D = c->diag[isp];
  if (!D.pending) return 0;
  double *h = nullptr;
  if (int rc = pinned(c, DiagSlots::len(c, false), &h)) return rc;
  const DiagSlots at(c, h);
  if (D.blocks > 0)
    HIP_TRY(hipMemcpyAsync(at.part, diag_part_dev(c, isp), sizeof(double) * DIAG_PART * D.blocks, hipMemcpyDeviceToHost, c->st));
  if (int rc = enqueue_tail_sums(c, isp, at)) return rc;
  if (D.blocks + diag_tail_blocks(c, isp) > 0) HIP_TRY(hipStreamSynchronize(c->st));
  return diag_collect(c, isp, at, false);
}

// ---------------------------------------------------------------------------
// kind 1 of the diagnostics sum (pic1dp_hip_set_diag_sum; kernels.hpp DiagFxArgs)
// ---------------------------------------------------------------------------
static const char *const kDfxNames[6] = {"markr", "total", "pertb", "sum v^2", "sum v^2 p", "sum v^2 w"};

// the exact pass over species isp into its slot of d_dfx: the markers' histograms and kinetic terms, then the tail
// slots' kinetic terms (the reference sums the whole local vector; slots beyond np live in set 0)
static int run_diag_pass_exact(pic1dp_ctx *c, int isp) {
  const pic1dp_input &in = c->in;
  Species &S = c->sp[isp];
  const PSet &A = S.set[c->cur];
  const size_t words = diag_fx_words(in.nx_opd, in.nv_opd);
  DiagFxArgs a{};
  a.acc = c->d_dfx + words * isp;
  for (int k = 0; k < 6; ++k) a.inv_q[k] = std::ldexp(1.0, -c->dfx_e[isp][k]);
  HIP_TRY(hipMemsetAsync(a.acc, 0, sizeof(long long) * words, c->st));
  if (S.np > 0)
    HIP_TRY(launch_ptcldist_exact(A.x, A.v, S.p, A.w, S.np, dist_geom(c), in.deltaf == 1, a,
                                  diag_launch(1, S.np, in.nx_opd, in.nv_opd, c->num_cu), c->cfg.dyn_tail, c->st));
  HIP_TRY(launch_energy_sums_exact(S.set[0].v, S.p, in.deltaf ? S.set[0].w : nullptr, S.np, S.nalloc - S.np, a,
                                   in.nx_opd * in.nv_opd, c->st));
  diag_note_pass(c, isp, 0, false, true);
  return 0;
}

// a pass of kind 1 if nothing has seen these markers yet
static int dfx_refresh(pic1dp_ctx *c, int isp) {
  return c->diag[isp].version == c->state_version ? 0 : run_diag_pass_exact(c, isp);
}

// Species isp's limbs and its counters of terms not summed on the host (out: diag_fx_words), from the cached pass or
// a new one: this rank's, or (reduced, with a communicator) the limbs summed over the ranks as int64.  A pass that left
// terms out is an error for every call it serves, until the markers change.
static int dfx_limbs_host(pic1dp_ctx *c, int isp, bool reduced, std::vector<long long> &out) {
  const pic1dp_input &in = c->in;
  if (int rc = diag_buffers(c)) return rc;
  const size_t words = diag_fx_words(in.nx_opd, in.nv_opd), limbs = diag_fx_limbs(in.nx_opd, in.nv_opd);
  if (!c->d_dfx) HIP_TRY(c->mem.alloc(&c->d_dfx, words * (in.nspecies + 1)));
  if (int rc = dfx_refresh(c, isp)) return rc;
  const long long *src = c->d_dfx + words * isp;
  if (reduced && c->comm) {  // reduce a copy: the cached local limbs stay local
    long long *red = c->d_dfx + words * in.nspecies;
    HIP_TRY(hipMemcpyAsync(red, src, sizeof(long long) * words, hipMemcpyDeviceToDevice, c->st));
    ncclResult_t r = rccl().AllReduce(red, red, limbs, ncclInt64, ncclSum, c->comm, c->st);
    if (r != ncclSuccess) return fail(PIC1DP_ERR_COMM, "ncclAllReduce: %s", rccl().GetErrorString(r));
    src = red;
  } else if (reduced && c->lay.nranks > 1) {
    return fail(PIC1DP_ERR_STATE, "nranks > 1 but no communicator: take diag_local_exact and reduce the limbs on the host");
  }
  out.resize(words);
  HIP_TRY(hipMemcpyAsync(out.data(), src, sizeof(long long) * words, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  const long long *rej = out.data() + limbs;
  if (c->diag[isp].pending) {
    for (int k = 0; k < 6; ++k) c->cnt.dfx_rejected += rej[k];
    c->diag[isp].pending = false;
  }
  for (int k = 0; k < 6; ++k)
    if (rej[k] != 0)
      return fail(PIC1DP_ERR_ARG,
                  "exact diagnostics sum: %lld term(s) of species %d, plane %s, lay beyond 2^%d quanta of 2^%d (|p|, |w| or |v| far "
                  "past the bounds the input gives) and were not summed; the diagnostics are incomplete",
                  rej[k], isp, kDfxNames[k], k < 3 ? 44 : 62, c->dfx_e[isp][k]);
  return 0;
}

// limbs -> the raw sums of the pass: every bin's total converted once (fx_limbs.hpp) and times 2^e; the v histograms are
// the integer row sums over ix of the planes.  dist: [3 nxv + 3 nv_opd] as ptcldist(finish = 0), or null
static void dfx_convert(const pic1dp_input &in, const int32_t e[6], const int64_t *limbs, double *sums, double *dist) {
  const int nxo = in.nx_opd, nvo = in.nv_opd;
  const size_t nxv = static_cast<size_t>(nxo) * nvo;
  for (int k = 0; k < 3 && dist; ++k) {
    const int64_t *hi = limbs + 2 * k * nxv, *lo = hi + nxv;
    const double q = std::ldexp(1.0, e[k]);
    fx_row_to_double(hi, lo, nxv, q, dist + k * nxv);
    for (int iv = 0; iv < nvo; ++iv) {
      int64_t H, L;
      fx_row_sum(hi + static_cast<size_t>(iv) * nxo, lo + static_cast<size_t>(iv) * nxo, nxo, &H, &L);
      fx_row_to_double(&H, &L, 1, q, dist + 3 * nxv + static_cast<size_t>(k) * nvo + iv);
    }
  }
  for (int k = 0; k < 3 && sums; ++k)
    fx_row_to_double(limbs + 6 * nxv + 2 * k, limbs + 6 * nxv + 2 * k + 1, 1, std::ldexp(1.0, e[3 + k]), sums + k);
}

// what the calls of kind 1 serve from: the raw kinetic sums and / or histograms of species isp
static int dfx_serve(pic1dp_ctx *c, int isp, bool reduced, double *sums, double *dist) {
  std::vector<long long> limbs;
  if (int rc = dfx_limbs_host(c, isp, reduced, limbs)) return rc;
  static_assert(sizeof(long long) == sizeof(int64_t), "limbs are 64-bit");
  dfx_convert(c->in, c->dfx_e[isp], reinterpret_cast<const int64_t *>(limbs.data()), sums, dist);
  return 0;
}


}  // namespace pic1dp_host

extern "C" {

int pic1dp_hip_energy_sums(pic1dp_ctx *c, int32_t isp, double out[3]) {
  CHECK_CTX(c);
  if (isp < 0 || isp >= c->in.nspecies || !out) return fail(PIC1DP_ERR_ARG, "bad argument");
  if (int rc = require_loaded(c)) return rc;
  if (c->diag_sum == 1) {
    if (int rc = dfx_serve(c, isp, false, out, nullptr)) return rc;
  } else {
    if (int rc = ensure_diag(c, isp)) return rc;
    for (int k = 0; k < 3; ++k) out[k] = c->diag[isp].sums[k];
  }
  if (!c->in.deltaf) out[2] = out[1];
  return 0;
}

// ---------------------------------------------------------------------------
// diagnostics of output_all
// ---------------------------------------------------------------------------
int pic1dp_hip_output_scalars(pic1dp_ctx *c, double *out, int32_t n) {
  CHECK_CTX(c);
  const int ns = c->in.nspecies;
  if (!out || n != 2 + 3 * ns) return fail(PIC1DP_ERR_ARG, "out must hold 2 + 3*nspecies doubles");
  std::vector<double> sums(3 * ns);
  if (c->diag_sum == 1) {  // the limbs summed over the ranks as integers, then converted: every rank forms the same doubles
    if (int rc = require_loaded(c)) return rc;
    for (int s = 0; s < ns; ++s) {
      if (int rc = dfx_serve(c, s, c->comm != nullptr, &sums[3 * s], nullptr)) return rc;
      if (!c->in.deltaf) sums[3 * s + 2] = sums[3 * s + 1];
    }
    return pic1dp_hip_output_scalars_from(c, sums.data(), out, n);
  }
  for (int s = 0; s < ns; ++s)
    if (int rc = pic1dp_hip_energy_sums(c, s, &sums[3 * s])) return rc;
  if (c->comm) {  // VecSum's scalar all-reduce
    double *d = c->d_scratch;
    HIP_TRY(hipMemcpyAsync(d, sums.data(), sizeof(double) * 3 * ns, hipMemcpyHostToDevice, c->st));
    if (int rc = allreduce_doubles(c, d, 3 * ns)) return rc;
    HIP_TRY(hipStreamSynchronize(c->st));
    HIP_TRY(hipMemcpy(sums.data(), d, sizeof(double) * 3 * ns, hipMemcpyDeviceToHost));
  }
  return pic1dp_hip_output_scalars_from(c, sums.data(), out, n);
}

// realbuf of output_field (src/pic1dp_output.F90:117-175) from the kinetic sums over all ranks and int E^2 dx
static void fill_scalars(const pic1dp_ctx *c, const double *sums, double energy, double *out) {
  const int ns = c->in.nspecies;
  out[0] = c->time;
  out[1] = energy;
  const pic1dp_input &in = c->in;
  for (int s = 0; s < ns; ++s) {
    double marker = sums[3 * s], total = sums[3 * s + 1], pert;
    if (in.deltaf == 1) {
      pert = sums[3 * s + 2];
      if (in.linear == 1) total = total + pert;  // :152-155
    } else {                                      // :156-170
      pert = total;
      if (in.iptcldist == 1) {
        pert = pert - 3.0 * in.species_density[s] * in.lx;
      } else if (in.iptcldist == 0) {
        pert = pert - in.species_temperature[s] / in.species_mass[s] * in.species_density[s] * in.lx;
      }
    }
    out[2 + 3 * s] = marker;
    out[3 + 3 * s] = total;
    out[4 + 3 * s] = pert;
  }
}

int pic1dp_hip_output_scalars_from(pic1dp_ctx *c, const double *sums, double *out, int32_t n) {
  CHECK_CTX(c);
  const int ns = c->in.nspecies;
  if (!sums || !out || n != 2 + 3 * ns) return fail(PIC1DP_ERR_ARG, "sums must hold 3*nspecies and out 2 + 3*nspecies doubles");
  double energy = 0.0;
  if (int rc = pic1dp_hip_field_energy(c, &energy)) return rc;
  fill_scalars(c, sums, energy, out);
  return 0;
}

// equilibrium f0(v) as the full-f branch of output_ptcldist normalises it
// (src/pic1dp_output.F90:375-451; note the reference divides by T/m, not sqrt(T/m))
static double output_f0(const pic1dp_input &in, int s, double sv) {
  const double T = in.species_temperature[s], T2 = in.species_temperature2[s], m = in.species_mass[s];
  const double den = in.species_density[s], v0 = in.species_v0[s];
  if (in.iptcldist == 1) return den * (sv * sv) * std::exp(-(sv * sv) / 2.0) / std::sqrt(2.0 * kPi);
  if (in.iptcldist == 2)
    return den * (std::exp(-((sv + v0) * (sv + v0)) / (2.0 * T / m)) + std::exp(-((sv - v0) * (sv - v0)) / (2.0 * T / m))) /
           (std::sqrt(8.0 * kPi) * T / m);
  if (in.iptcldist == 3)
    return den * std::exp(-(sv * sv) / (2.0 * T / m)) / (std::sqrt(2.0 * kPi) * T / m) +
           (1.0 - den) * std::exp(-((sv - v0) * (sv - v0)) / (2.0 * T2 / m)) / (std::sqrt(2.0 * kPi) * T2 / m);
  return den * std::exp(-((sv - v0) * (sv - v0)) / (2.0 * T / m)) / (std::sqrt(2.0 * kPi) * T / m);
}

// what output_ptcldist does with the sums over ranks (src/pic1dp_output.F90:328-331, :361-453): linear total +=
// pertb, scaling by the histogram cell sizes, full-f pertb = total - f0; in place on host arrays
static void finish_ptcldist(const pic1dp_input &in, int isp, double *mxv, double *txv, double *pxv, double *mv, double *tv,
                            double *pv) {
  const int nxo = in.nx_opd, nvo = in.nv_opd;
  const size_t nxv = static_cast<size_t>(nxo) * nvo;
  if (in.linear == 1) {  // :328-331
    for (size_t i = 0; i < nxv; ++i) txv[i] = txv[i] + pxv[i];
    for (int i = 0; i < nvo; ++i) tv[i] = tv[i] + pv[i];
  }
  const double delv_inv = static_cast<double>(nvo - 1) / (2.0 * in.v_max);  // :203-205
  const double delx_inv = static_cast<double>(nxo) / in.lx;
  for (size_t i = 0; i < nxv; ++i) {
    mxv[i] = mxv[i] * delx_inv * delv_inv;
    txv[i] = txv[i] * delx_inv * delv_inv;
  }
  for (int i = 0; i < nvo; ++i) {
    mv[i] = mv[i] * delv_inv;
    tv[i] = tv[i] * delv_inv;
  }
  if (in.deltaf == 1) {
    for (size_t i = 0; i < nxv; ++i) pxv[i] = pxv[i] * delx_inv * delv_inv;
    for (int i = 0; i < nvo; ++i) pv[i] = pv[i] * delv_inv;
  } else {  // :370-453
    for (int iv = 0; iv < nvo; ++iv) {
      const double sv = (static_cast<double>(iv) / static_cast<double>(nvo - 1) * 2.0 - 1.0) * in.v_max;
      const double f0 = output_f0(in, isp, sv);
      for (int ix = 0; ix < nxo; ++ix) pxv[static_cast<size_t>(iv) * nxo + ix] = txv[static_cast<size_t>(iv) * nxo + ix] - f0;
      pv[iv] = tv[iv] - in.lx * f0;
    }
  }
}

// the six arrays of a raw [3 nx_opd nv_opd + 3 nv_opd] block: markr_xv, total_xv, pertb_xv, markr_v, total_v, pertb_v
static void dist_split(const pic1dp_input &in, double *raw, double *a[6]) {
  const size_t nxv = static_cast<size_t>(in.nx_opd) * in.nv_opd;
  for (int k = 0; k < 6; ++k) a[k] = raw + (k < 3 ? k * nxv : 3 * nxv + (k - 3) * static_cast<size_t>(in.nv_opd));
}
static void finish_ptcldist(const pic1dp_input &in, int isp, double *raw) {
  double *a[6];
  dist_split(in, raw, a);
  finish_ptcldist(in, isp, a[0], a[1], a[2], a[3], a[4], a[5]);
}

int pic1dp_hip_ptcldist(pic1dp_ctx *c, int32_t isp, int32_t finish, double *markr_xv, double *total_xv,
                        double *pertb_xv, double *markr_v, double *total_v, double *pertb_v) {
  CHECK_CTX(c);
  if (isp < 0 || isp >= c->in.nspecies) return fail(PIC1DP_ERR_ARG, "bad species index");
  if (int rc = require_loaded(c)) return rc;
  const pic1dp_input &in = c->in;
  const size_t ntot = dist_len(in);
  // either kind: the raw block of the species on the host, summed over the ranks where the caller wants it finished
  double *raw = nullptr;
  std::vector<double> converted;
  if (c->diag_sum == 1) {
    if (finish && !c->comm && c->lay.nranks > 1)
      return fail(PIC1DP_ERR_STATE, "nranks > 1 but no communicator: take diag_local_exact and reduce the limbs on the host");
    converted.resize(ntot);
    raw = converted.data();
    if (int rc = dfx_serve(c, isp, finish && c->comm, nullptr, raw)) return rc;
  } else {
    if (int rc = ensure_diag(c, isp)) return rc;
    const double *hist = c->d_dist + ntot * isp;
    if (finish && c->comm) {  // reduce a copy: the cached local histograms stay local
      double *red = c->d_dist + ntot * in.nspecies;
      HIP_TRY(hipMemcpyAsync(red, hist, sizeof(double) * ntot, hipMemcpyDeviceToDevice, c->st));
      if (int rc = allreduce_doubles(c, red, ntot)) return rc;
      hist = red;
    } else if (finish && c->lay.nranks > 1) {
      return fail(PIC1DP_ERR_STATE, "nranks > 1 but no communicator: take finish = 0 and reduce the local sums on the host");
    }
    if (int rc = pinned(c, ntot, &raw)) return rc;
    HIP_TRY(hipMemcpyAsync(raw, hist, sizeof(double) * ntot, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
  }
  if (finish) finish_ptcldist(in, isp, raw);
  double *src[6], *dst[6] = {markr_xv, total_xv, pertb_xv, markr_v, total_v, pertb_v};
  dist_split(in, raw, src);
  for (int k = 0; k < 6; ++k)
    if (dst[k]) std::memcpy(dst[k], src[k], sizeof(double) * (k < 3 ? static_cast<size_t>(in.nx_opd) * in.nv_opd : static_cast<size_t>(in.nv_opd)));
  return 0;
}

int pic1dp_hip_ptcldist_finish(pic1dp_ctx *c, int32_t isp, double *markr_xv, double *total_xv, double *pertb_xv,
                               double *markr_v, double *total_v, double *pertb_v) {
  CHECK_CTX(c);
  if (isp < 0 || isp >= c->in.nspecies) return fail(PIC1DP_ERR_ARG, "bad species index");
  if (!markr_xv || !total_xv || !pertb_xv || !markr_v || !total_v || !pertb_v) return fail(PIC1DP_ERR_ARG, "null array");
  finish_ptcldist(c->in, isp, markr_xv, total_xv, pertb_xv, markr_v, total_v, pertb_v);
  return 0;
}


// output_all's pinned record: [E | cd | re | im | energy + pad], then per species its DiagSlots with the histograms
struct RecordLayout {
  size_t nx, nm, cd, re, im, energy, species, per_species, total;   // (E at 0)
  explicit RecordLayout(const pic1dp_ctx *c)
      : nx(c->in.nx), nm(c->in.nmode), cd(nx), re(2 * nx), im(re + nm), energy(im + nm), species(energy + 8),
        per_species(DiagSlots::len(c, true)), total(species + per_species * c->in.nspecies) {}
  DiagSlots slots(const pic1dp_ctx *c, double *h, int s) const { return DiagSlots(c, h + species + per_species * s); }
};

// output_all, enqueued: the passes of the species nothing has seen yet, int E^2 dx, the record gathered on the device and
// sent in ONE transfer (every small copy of its own costs the stream ~10 us), the tail slots' sums behind it
static int enqueue_record(pic1dp_ctx *c, const RecordLayout &L, double *h, bool with_hist) {
  const int ns = c->in.nspecies;
  const size_t ntot = dist_len(c->in);
  for (int s = 0; s < ns; ++s)
    if (int rc = diag_refresh(c, s)) return rc;
  double *slot = c->d_scratch + kEnergyBlocks * 3;
  HIP_TRY(launch_field_energy(c->d_E, c->in.nx, c->in.lx, static_cast<double>(c->in.nx), slot, c->st));
  if (c->d_rec_doubles < L.total) {
    c->d_rec_doubles = 0;
    HIP_TRY(c->mem.regrow(&c->d_rec, L.total));
    c->d_rec_doubles = L.total;
  }
  PackArgs pk{};
  auto seg = [&pk](const double *src, size_t dst, size_t n) {
    if (n == 0) return;
    pk.src[pk.count] = src, pk.dst[pk.count] = static_cast<unsigned>(dst), pk.n[pk.count] = static_cast<unsigned>(n);
    pk.count++;
  };
  seg(c->d_E, 0, L.nx);
  seg(c->d_chargeden, L.cd, L.nx);
  seg(c->d_mode_re, L.re, L.nm);
  seg(c->d_mode_im, L.im, L.nm);
  seg(slot, L.energy, 1);
  for (int s = 0; s < ns; ++s) {
    const DiagSlots at = L.slots(c, h, s);
    if (c->diag[s].pending) seg(diag_part_dev(c, s), at.part - h, static_cast<size_t>(DIAG_PART) * c->diag[s].blocks);
    if (with_hist) seg(c->d_dist + ntot * s, at.hist - h, ntot);
  }
  HIP_TRY(launch_pack_record(pk, c->d_rec, c->st));
  HIP_TRY(hipMemcpyAsync(h, c->d_rec, sizeof(double) * L.total, hipMemcpyDeviceToHost, c->st));
  for (int s = 0; s < ns; ++s)  // (unloaded or emptied slots)
    if (int rc = enqueue_tail_sums(c, s, L.slots(c, h, s))) return rc;
  return 0;
}

// output_all, settled: the record has arrived -- the species' passes collected, the scalars formed, everything handed out
static int settle_record(pic1dp_ctx *c, const RecordLayout &L, double *h, double *scalars, double *E, double *cd, double *re,
                         double *im, double *dist) {
  const pic1dp_input &in = c->in;
  const int ns = in.nspecies;
  const size_t ntot = dist_len(in);
  std::vector<double> sums(3 * static_cast<size_t>(ns));
  for (int s = 0; s < ns; ++s) {
    if (int rc = diag_collect(c, s, L.slots(c, h, s), dist != nullptr)) return rc;
    for (int k = 0; k < 3; ++k) sums[3 * s + k] = c->diag[s].sums[k];
    if (!in.deltaf) sums[3 * s + 2] = sums[3 * s + 1];
  }
  fill_scalars(c, sums.data(), h[L.energy], scalars);
  if (E) std::memcpy(E, h, sizeof(double) * L.nx);
  if (cd) std::memcpy(cd, h + L.cd, sizeof(double) * L.nx);
  if (re) std::memcpy(re, h + L.re, sizeof(double) * L.nm);
  if (im) std::memcpy(im, h + L.im, sizeof(double) * L.nm);
  for (int s = 0; s < ns && dist; ++s) {
    double *d = L.slots(c, h, s).hist;
    finish_ptcldist(in, s, d);
    std::memcpy(dist + ntot * s, d, sizeof(double) * ntot);
  }
  return 0;
}

// Everything output_all writes (src/pic1dp_output.F90:100-189, 196-477) in ONE call and one wait: the diagnostics passes of
// all species, int E^2 dx, and every transfer to the host enqueued behind them on the engine's stream through the pinned
// staging (the separate calls wait three times and more per record: 0.16 ms of host time that is most of what a record
// costs at 6.4e6 markers).  dist: [nspecies][3 nx_opd nv_opd + 3 nv_opd] as output_ptcldist writes them (finished), or null.
// Several ranks: composed of the separate calls, which own the reductions.
int pic1dp_hip_output_all(pic1dp_ctx *c, double *scalars, int32_t nscal, double *E, double *cd, double *re, double *im,
                          double *dist) {
  CHECK_CTX(c);
  const pic1dp_input &in = c->in;
  const int ns = in.nspecies;
  if (!scalars || nscal != 2 + 3 * ns) return fail(PIC1DP_ERR_ARG, "scalars must hold 2 + 3*nspecies doubles");
  if (c->comm || c->lay.nranks > 1 || c->diag_sum == 1) {  // (kind 1 of the diagnostics sum: served by the separate calls)
    if (int rc = pic1dp_hip_output_scalars(c, scalars, nscal)) return rc;
    if (int rc = pic1dp_hip_get_field(c, E, cd, re, im)) return rc;
    for (int s = 0; s < ns && dist; ++s) {
      double *d[6];
      dist_split(in, dist + dist_len(in) * s, d);
      if (int rc = pic1dp_hip_ptcldist(c, s, 1, d[0], d[1], d[2], d[3], d[4], d[5])) return rc;
    }
    return 0;
  }
  if (int rc = call_site(c, cd ? Call::OutputAllCd : Call::OutputAll)) return rc;
  if (int rc = diag_buffers(c)) return rc;
  const RecordLayout L(c);
  double *h = nullptr;
  if (int rc = pinned(c, L.total, &h)) return rc;
  if (int rc = enqueue_record(c, L, h, dist != nullptr)) return rc;
  HIP_TRY(hipStreamSynchronize(c->st));
  if (int rc = xchg_check(c)) return rc;
  return settle_record(c, L, h, scalars, E, cd, re, im, dist);
}

// ---------------------------------------------------------------------------
// kind 1 of the diagnostics sum: the switch, the quanta, the split phase
// ---------------------------------------------------------------------------
int pic1dp_hip_diag_quanta(const pic1dp_input *in, int32_t ispecies, int32_t log2_quantum[6]) {
  if (!in || !log2_quantum) return fail(PIC1DP_ERR_ARG, "null argument");
  int32_t e = 0;
  if (int rc = pic1dp_hip_charge_quantum(in, ispecies, &e)) return rc;
  const int kb = e + 52;  // |p|, |w| <= 2^kb
  const double v2 = in->v_max * in->v_max;
  if (!(v2 > 0.0) || !std::isfinite(v2)) return fail(PIC1DP_ERR_ARG, "v_max must be positive and finite");
  const int kv = ceil_log2(v2);
  log2_quantum[0] = -40;
  log2_quantum[1] = log2_quantum[2] = kb - 40;
  log2_quantum[3] = kv - 52;
  log2_quantum[4] = log2_quantum[5] = kv + kb - 52;
  return 0;
}

int pic1dp_hip_diag_quantise(double term, int32_t log2_quantum, int32_t kinetic, int64_t *n) {
  if (!n) return fail(PIC1DP_ERR_ARG, "null argument");
  long long q = 0;
  if (!diag_fx_quantise(term, std::ldexp(1.0, -log2_quantum), kinetic ? FX_LIMIT : DIAG_FX_LIMIT, &q))
    return fail(PIC1DP_ERR_ARG, "a term of 2^%d quanta or more is not summed", kinetic ? 62 : 44);
  *n = q;
  return 0;
}

int pic1dp_hip_set_diag_sum(pic1dp_ctx *c, int32_t kind) {
  CHECK_CTX(c);
  if (kind != 0 && kind != 1) return fail(PIC1DP_ERR_ARG, "diagnostics sum must be 0 (FP64 and per-pass fixed point) or 1 (exact)");
  if (c->fused_pending) return fail(PIC1DP_ERR_STATE, "set_diag_sum while a push, a charge or a solve is pending: call it between time steps");
  if (int rc = call_site(c, Call::BetweenSteps, "set_diag_sum")) return rc;
  if (kind == 1)
    for (int s = 0; s < c->in.nspecies; ++s)
      if (int rc = pic1dp_hip_diag_quanta(&c->in, s, c->dfx_e[s])) return rc;
  // the cached diagnostics belong to the other kind
  for (DiagSpecies &D : c->diag) D.version = 0, D.pending = false;
  c->diag_sum = kind;
  return 0;
}

int pic1dp_hip_diag_limbs_len(pic1dp_ctx *c, int64_t *n) {
  CHECK_CTX(c);
  if (!n) return fail(PIC1DP_ERR_ARG, "null argument");
  *n = static_cast<int64_t>(diag_fx_limbs(c->in.nx_opd, c->in.nv_opd));
  return 0;
}

int pic1dp_hip_diag_local_exact(pic1dp_ctx *c, int32_t isp, int64_t *limbs) {
  CHECK_CTX(c);
  if (isp < 0 || isp >= c->in.nspecies || !limbs) return fail(PIC1DP_ERR_ARG, "bad argument");
  if (c->diag_sum != 1) return fail(PIC1DP_ERR_STATE, "diag_local_exact needs set_diag_sum(1)");
  if (int rc = require_loaded(c)) return rc;
  std::vector<long long> w;
  if (int rc = dfx_limbs_host(c, isp, false, w)) return rc;
  std::memcpy(limbs, w.data(), sizeof(int64_t) * diag_fx_limbs(c->in.nx_opd, c->in.nv_opd));
  return 0;
}

int pic1dp_hip_diag_convert(const pic1dp_input *in, int32_t isp, const int64_t *limbs, double sums[3], double *dist) {
  if (!in || !limbs) return fail(PIC1DP_ERR_ARG, "null argument");
  int32_t e[6];
  if (int rc = pic1dp_hip_diag_quanta(in, isp, e)) return rc;
  if (in->nx_opd < 1 || in->nv_opd < 2) return fail(PIC1DP_ERR_ARG, "nx_opd >= 1 and nv_opd >= 2 required");
  dfx_convert(*in, e, limbs, sums, dist);
  if (sums && !in->deltaf) sums[2] = sums[1];
  return 0;
}

int pic1dp_hip_diag_convert_exact(pic1dp_ctx *c, int32_t isp, const int64_t *limbs, double sums[3], double *dist) {
  CHECK_CTX(c);
  return pic1dp_hip_diag_convert(&c->in, isp, limbs, sums, dist);
}

}  // extern "C"
