// exact_charge.cpp -- kind 1 of the charge sum: a deposit whose result does not depend on the order
// of its additions.  The quantum rule (pic1dp_hip_charge_quantum), the switch (pic1dp_hip_set_charge_sum), the settle
// step that turns the integer accumulators into the species accumulators, and the overflow report.  The kernels:
// device_math.hpp RhoFx (deposit, flush), kernels_field.hip k_fx_* (normalise, exchange, conversion).
#include "ctx.hpp"
#include "fx_limbs.hpp"

namespace pic1dp_host {

namespace {

// a bound on |p| and |w| of the species' markers as the loader makes them (loader.cpp): the marker prefactor times
// the distribution's peak, times (1 + sum of |perturbation amplitudes|) -- w = amp p, and a non-linear run adds w to p
double marker_bound(const pic1dp_input &in, int isp) {
  const double T = in.species_temperature[isp], T2 = in.species_temperature2[isp];
  const double m = in.species_mass[isp], den = in.species_density[isp];
  const double ninit = static_cast<double>(in.species_nparticle_init[isp]);
  double amp = 0.0;
  for (int j = 0; j < in.init_nmode; ++j) amp += std::fabs(in.init_mode_cos[j]) + std::fabs(in.init_mode_sin[j]);
  double base;
  if (in.imarker == 1) {
    base = std::fabs(den * in.lx / ninit);
  } else {
    const int dist = in.iptcldist;
    const double pref = std::fabs((dist == 3 ? 1.0 : den) * in.lx * 2.0 * in.v_max / ninit);
    const double g1 = std::sqrt(2.0 * kPi * T / m), g2 = std::sqrt(2.0 * kPi * T2 / m);
    const double g8 = std::sqrt(8.0 * kPi * T / m), gs = std::sqrt(2.0 * kPi);
    double peak;
    switch (dist) {
      case 1: peak = 1.0 / gs; break;                                       // q exp(-q/2) <= 2/e < 1
      case 2: peak = 2.0 / g8; break;                                       // two exp <= 1 each
      case 3: peak = std::fabs(den) / g1 + std::fabs(1.0 - den) / g2; break;
      default: peak = 1.0 / g1;
    }
    base = pref * peak;
  }
  // (1 + 2^-20: the loader's own roundings on the way to p and w)
  return base * (1.0 + amp) * (1.0 + 0x1p-20);
}

}  // namespace

FxArgs fx_args(const pic1dp_ctx *c, int isp) {
  FxArgs f{};
  if (c->charge_sum != 1) return f;
  f.acc = c->d_fx + static_cast<size_t>(isp) * 2 * c->in.nx;
  f.inv_q = c->fx_inv_q[isp];
  f.ovf = c->h_fx_ovf + isp;
  return f;
}

// The deposits of a collect_charge / sub-step in d_fx: summed over the ranks (integers: RCCL int64, the exchange, or --
// charge_reduced_exact -- the host), converted into the species accumulators' copy 0.  What follows reads them as on
// one rank (k_charge_local / chargeden with the species sum): every rank forms the same doubles from the same integers.
int fx_settle(pic1dp_ctx *c) {
  const int ns = c->in.nspecies, nx = c->in.nx;
  if (several_ranks(c)) {
    Span sp(c->tm, PIC1DP_IWT_MPIALLREDU, c->tm.timers_on);
    if (xchg_active(c)) {
      HIP_TRY(launch_fx_exchange(c->d_fx, ns, nx, next_xchg_args(c), c->st));
    } else if (c->comm) {
      HIP_TRY(launch_fx_normalise(c->d_fx, ns, nx, c->st));
      ncclResult_t r = rccl().AllReduce(c->d_fx, c->d_fx, static_cast<size_t>(2) * ns * nx, ncclInt64, ncclSum, c->comm, c->st);
      if (r != ncclSuccess) return fail(PIC1DP_ERR_COMM, "ncclAllReduce: %s", rccl().GetErrorString(r));
    } else {
      return fail(PIC1DP_ERR_STATE, "nranks > 1 but no communicator: call pic1dp_hip_comm_init, connect the one-hop exchange, "
                                    "or use charge_local_exact/charge_reduced_exact");
    }
    if (int rc = sp.end()) return rc;
  }
  HIP_TRY(launch_fx_to_rho(c->d_fx, c->fa.rho_sp, ns, nx, c->fx_q, c->st));
  return 0;
}

int fx_check(pic1dp_ctx *c) {
  if (!c->h_fx_ovf) return 0;
  for (int s = 0; s < c->in.nspecies; ++s) {
    const unsigned long long v = reinterpret_cast<volatile unsigned long long *>(c->h_fx_ovf)[s];
    if (v > c->fx_ovf_seen[s]) {
      const unsigned long long n = v - c->fx_ovf_seen[s];
      c->fx_ovf_seen[s] = v;
      return fail(PIC1DP_ERR_ARG,
                  "exact charge sum: %llu contribution(s) of species %d lay beyond 2^62 quanta of 2^%d (|w| or |p| far past "
                  "the bound the input gives) and were not summed; the charge is incomplete",
                  n, s, c->fx_e[s]);
    }
  }
  return 0;
}

}  // namespace pic1dp_host

extern "C" {

int pic1dp_hip_charge_quantum(const pic1dp_input *in, int32_t ispecies, int32_t *log2_quantum) {
  if (!in || !log2_quantum) return fail(PIC1DP_ERR_ARG, "null argument");
  if (in->abi_version != PIC1DP_ABI_VERSION) return fail(PIC1DP_ERR_ARG, "abi_version %d, expected %d", in->abi_version, PIC1DP_ABI_VERSION);
  if (in->nspecies < 1 || in->nspecies > PIC1DP_MAX_SPECIES || ispecies < 0 || ispecies >= in->nspecies)
    return fail(PIC1DP_ERR_ARG, "species %d of %d", ispecies, in->nspecies);
  if (in->init_nmode < 0 || in->init_nmode > PIC1DP_MAX_INIT_MODES) return fail(PIC1DP_ERR_ARG, "init_nmode out of range");
  const double b = marker_bound(*in, ispecies);
  if (!std::isfinite(b)) return fail(PIC1DP_ERR_ARG, "species %d: no finite bound on its markers' weights", ispecies);
  if (!(b > 0.0)) {  // (no weight at all: any quantum sums zeros exactly)
    *log2_quantum = -52;
    return 0;
  }
  *log2_quantum = ceil_log2(b) - 52;
  return 0;
}

int pic1dp_hip_set_charge_sum(pic1dp_ctx *c, int32_t kind) {
  CHECK_CTX(c);
  if (kind != 0 && kind != 1) return fail(PIC1DP_ERR_ARG, "charge sum must be 0 (FP64 atomics) or 1 (exact)");
  if (c->fused_pending) return fail(PIC1DP_ERR_STATE, "set_charge_sum while a push, a charge or a solve is pending: call it between time steps");
  if (int rc = call_site(c, Call::BetweenSteps, "set_charge_sum")) return rc;
  if (kind == 1) {
    for (int s = 0; s < c->in.nspecies; ++s) {
      int32_t e = 0;
      if (int rc = pic1dp_hip_charge_quantum(&c->in, s, &e)) return rc;
      c->fx_e[s] = e;
      c->fx_q[s] = std::ldexp(1.0, e);
      c->fx_inv_q[s] = std::ldexp(1.0, -e);
    }
    if (!c->d_fx) {
      const size_t words = 2 * static_cast<size_t>(c->in.nspecies) * c->in.nx;
      HIP_TRY(c->mem.alloc(&c->d_fx, words));
      HIP_TRY(hipMemsetAsync(c->d_fx, 0, sizeof(long long) * words, c->st));
    }
    if (!c->h_fx_ovf) {
      HIP_TRY(c->mem.alloc_pinned(&c->h_fx_ovf, 8));
      std::memset(c->h_fx_ovf, 0, 8 * sizeof(unsigned long long));
      std::memset(c->fx_ovf_seen, 0, sizeof c->fx_ovf_seen);
    }
    // a prediction the last one-pass step left: kind 1 does not use it (two passes per step), its sums go
    if (c->pred_version != 0 && c->d_pred_all)
      HIP_TRY(hipMemsetAsync(c->d_pred_all, 0, sizeof(double) * 3 * c->plan.pred_set_doubles, c->st));
    c->pred_version = 0;
  }
  c->charge_sum = kind;
  return 0;
}

}  // extern "C"
