// capi_checkpoint.cpp -- the state digest, checkpoint and restart behind the C ABI (include/pic1dp_hip.h).
// The file's format, its writer and reader are host code of their own (checkpoint.cpp: no HIP call); here the markers move
// between file and device through the context's pinned staging in chunks, and the context's state is gathered and restored.
#include <cstddef>

#include "checkpoint.hpp"
#include "ctx.hpp"

namespace {

constexpr int64_t kChunkDoubles = static_cast<int64_t>(4) << 20;  // 32 MiB of pinned staging per transfer

// the bases of array k (0 x, 1 v, 2 w, 3 p) of a species: where slots below np live now, and the tail slots (set 0)
void array_bases(const pic1dp_ctx *c, const Species &S, const double *cur[4], const double *first[4]) {
  const PSet &A = S.set[c->cur], &F = S.set[0];
  cur[0] = A.x, cur[1] = A.v, cur[2] = A.w, cur[3] = S.p;
  first[0] = F.x, first[1] = F.v, first[2] = F.w, first[3] = S.p;
}

// D[s][k] of the markers as they lie in memory: the digest kernel per species, one wait
int device_digests(pic1dp_ctx *c, uint64_t *out) {
  const int ns = c->in.nspecies;
  if (!c->d_digest) HIP_TRY(c->mem.alloc(&c->d_digest, static_cast<size_t>(4) * PIC1DP_MAX_SPECIES));
  HIP_TRY(hipMemsetAsync(c->d_digest, 0, sizeof(unsigned long long) * 4 * ns, c->st));
  for (int s = 0; s < ns; ++s) {
    const Species &S = c->sp[s];
    DigestArgs a{};
    array_bases(c, S, a.cur, a.first);
    a.np = S.np, a.nalloc = S.nalloc;
    a.out = c->d_digest + 4 * s;
    HIP_TRY(launch_state_digest(a, digest_launch(S.nalloc, c->num_cu), c->st));
  }
  double *h = nullptr;
  if (int rc = pinned(c, static_cast<size_t>(4) * ns, &h)) return rc;
  HIP_TRY(hipMemcpyAsync(h, c->d_digest, sizeof(unsigned long long) * 4 * ns, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  std::memcpy(out, h, sizeof(uint64_t) * 4 * ns);
  return 0;
}

// slots [off, off + n) of array k in logical order -> host
int pull_logical(pic1dp_ctx *c, const Species &S, int k, int64_t off, int64_t n, double *host) {
  const double *cur[4], *first[4];
  array_bases(c, S, cur, first);
  const int64_t nv = std::max<int64_t>(0, std::min(off + n, S.np) - off);  // of them below np
  if (int rc = get_range(c, cur[k], off, host, nv)) return rc;
  return get_range(c, first[k], off + nv, host + nv, n - nv);
}

struct InputField {
  const char *name;
  size_t off, len;
};
#define F(name) {#name, offsetof(pic1dp_input, name), sizeof(static_cast<pic1dp_input *>(nullptr)->name)}
const InputField kInputFields[] = {
    F(abi_version), F(ntime_max), F(linear), F(iptcldist), F(nspecies), F(nmode), F(init_nmode), F(deltaf), F(imarker), F(nx), F(nv),
    F(iptclshape), F(nx_opd), F(nv_opd), F(multirand_al_int), F(multirand_seed_type), F(multirand_warmup), F(multirand_selftest),
    F(nparticle_max), F(species_nparticle_init), F(time_max), F(lx), F(dt), F(v_max), F(output_interval), F(species_charge),
    F(species_mass), F(species_temperature), F(species_temperature2), F(species_density), F(species_v0), F(modes), F(init_mode),
    F(init_mode_cos), F(init_mode_sin), F(nmerge), F(nremove), F(nsplit), F(typeremove), F(split_ngroup), F(reserved0), F(remove_frac),
    F(split_dv_sig_frac), F(tmerge), F(thshmerge), F(tremove), F(thshremove), F(tsplit), F(thshsplit)};
#undef F

void context_settings(const pic1dp_ctx *c, int32_t out[ckpt::kNumSettings]) {
  out[0] = c->charge_sum, out[1] = c->diag_sum, out[2] = c->field_transform, out[3] = c->field_solver, out[4] = c->step_mode;
  out[5] = c->fuse_output, out[6] = c->seed_offset;
}

// the first thing in which the file's run differs from the context's, or null
const char *first_difference(const pic1dp_ctx *c, const ckpt::Small &f, char *buf, size_t nbuf) {
  const unsigned char *a = reinterpret_cast<const unsigned char *>(&c->in), *b = reinterpret_cast<const unsigned char *>(&f.in);
  for (const InputField &fld : kInputFields)
    if (std::memcmp(a + fld.off, b + fld.off, fld.len) != 0) {
      std::snprintf(buf, nbuf, "input field %s", fld.name);
      return buf;
    }
  if (f.rank != c->lay.rank) return "layout field rank";
  if (f.nranks != c->lay.nranks) return "layout field nranks";
  if (f.npe != c->lay.npe) return "layout field npe";
  int32_t mine[ckpt::kNumSettings];
  context_settings(c, mine);
  for (int k = 0; k < ckpt::kNumSettings; ++k)
    if (mine[k] != f.settings[k]) {
      std::snprintf(buf, nbuf, "setting %s (file %d, context %d)", ckpt::kSettingNames[k], f.settings[k], mine[k]);
      return buf;
    }
  if (f.nblk != c->plan.nblk) return "number of owned blocks";
  for (int s = 0; s < c->in.nspecies; ++s)
    if (f.nalloc[s] != c->sp[s].nalloc) {
      std::snprintf(buf, nbuf, "allocated slots of species %d", s);
      return buf;
    }
  return nullptr;
}

}  // namespace

extern "C" {

int pic1dp_hip_host_digest(const double *a, int64_t n, uint64_t *out) {
  if (!out || n < 0 || (!a && n > 0)) return fail(PIC1DP_ERR_ARG, "host_digest: null array or n < 0");
  uint64_t s = 0, g = DIGEST_GOLD;
  for (int64_t i = 0; i < n; ++i, g += DIGEST_GOLD) {
    uint64_t u;
    std::memcpy(&u, a + i, 8);
    s += digest_mix(u, g);
  }
  *out = s;
  return 0;
}

int pic1dp_hip_state_digest(pic1dp_ctx *c, uint64_t *out) {
  CHECK_CTX(c);
  if (!out) return fail(PIC1DP_ERR_ARG, "null output");
  if (!c->loaded) return fail(PIC1DP_ERR_STATE, "no particles: call particle_load or particles_upload first");
  if (int rc = call_site(c, Call::ReadMarkers)) return rc;   // (as particles_download: a noted push becomes memory; clean: nothing is launched)
  return device_digests(c, out);
}

int pic1dp_hip_checkpoint_write(pic1dp_ctx *c, const char *path) {
  CHECK_CTX(c);
  if (!path || !*path) return fail(PIC1DP_ERR_ARG, "checkpoint_write: no file name");
  if (c->fused_pending) return fail(PIC1DP_ERR_STATE, "internal: checkpoint_write with a fused solve pending");
  // between time steps only (no particles, a charge or a push pending, a call of the six the last: refused); what the
  // step's end still owes is settled; a half step's kept mode alone in field_chargeden: refused behind that
  if (int rc = call_site(c, Call::Checkpoint)) return rc;
  HIP_TRY(hipStreamSynchronize(c->st));
  if (int rc = xchg_check(c)) return rc;

  const pic1dp_input &in = c->in;
  const int ns = in.nspecies;
  const size_t nx = in.nx, nm = in.nmode;
  ckpt::Small f;
  f.in = in;
  f.rank = c->lay.rank, f.nranks = c->lay.nranks, f.npe = c->lay.npe, f.nblk = c->plan.nblk;
  context_settings(c, f.settings);
  f.itime = c->itime, f.time = c->time;
  f.imerge = c->imerge, f.iremove = c->iremove, f.isplit = c->isplit;
  f.rng_ready = c->rng_ready ? 1 : 0;
  f.rng_words = c->rng_ready ? Multirand::state_words() : 0;
  f.nalloc.resize(ns), f.np.resize(ns), f.blk_np.resize(ns), f.max_p.resize(ns), f.max_w.resize(ns), f.fixed.resize(ns);
  f.fxb.resize(4 * static_cast<size_t>(ns));
  for (int s = 0; s < ns; ++s) {
    f.nalloc[s] = c->sp[s].nalloc, f.np[s] = c->sp[s].np;
    f.blk_np[s] = c->blk_np[s];
    f.max_p[s] = c->diag[s].max_p, f.max_w[s] = c->diag[s].max_w, f.fixed[s] = c->diag[s].fixed ? 1 : 0;
    HIP_TRY(hipMemcpy(&f.fxb[4 * static_cast<size_t>(s)], c->sp[s].fxb, 32, hipMemcpyDeviceToHost));
  }
  f.E.resize(nx), f.cd.resize(nx), f.re.resize(nm), f.im.resize(nm);
  HIP_TRY(hipMemcpy(f.E.data(), c->d_E, 8 * nx, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(f.cd.data(), c->d_chargeden, 8 * nx, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(f.re.data(), c->d_mode_re, 8 * nm, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(f.im.data(), c->d_mode_im, 8 * nm, hipMemcpyDeviceToHost));
  f.hist.resize(static_cast<size_t>(c->hist_count));
  if (c->hist_count > 0) HIP_TRY(hipMemcpy(f.hist.data(), c->d_hist, 8 * f.hist.size(), hipMemcpyDeviceToHost));
  if (c->rng_ready) {
    f.rng.resize(c->plan.nblk);
    for (int b = 0; b < c->plan.nblk; ++b) c->blk_rng[b].export_state(&f.rng[b].engine, &f.rng[b].pos, &f.rng[b].held, &f.rng[b].val, &f.rng[b].q);
  }
  if (int rc = device_digests(c, &f.digest[0][0])) return rc;

  std::string err;
  ckpt::Writer w;
  if (w.begin(path, f, &err)) return fail(PIC1DP_ERR_ARG, "%s", err.c_str());
  double *h = nullptr;
  if (int rc = pinned(c, static_cast<size_t>(kChunkDoubles), &h)) return rc;
  for (int s = 0; s < ns; ++s)
    for (int k = 0; k < 4; ++k) {
      uint64_t d = 0;
      for (int64_t off = 0; off < f.nalloc[s]; off += kChunkDoubles) {
        const int64_t n = std::min(kChunkDoubles, f.nalloc[s] - off);
        if (int rc = pull_logical(c, c->sp[s], k, off, n, h)) return rc;   // (w's destructor removes the partial file)
        uint64_t g = static_cast<uint64_t>(off + 1) * DIGEST_GOLD;
        for (int64_t i = 0; i < n; ++i, g += DIGEST_GOLD) {
          uint64_t u;
          std::memcpy(&u, h + i, 8);
          d += digest_mix(u, g);
        }
        if (w.markers(h, n, &err)) return fail(PIC1DP_ERR_ARG, "%s", err.c_str());
      }
      if (d != f.digest[s][k])   // what went into the file against what the kernel saw on the device
        return fail(PIC1DP_ERR_HIP, "checkpoint_write: species %d, array %s: what crossed to the host does not have the digest the device computed",
                    s, ckpt::kArrayNames[k]);
    }
  if (w.finish(f, &err)) return fail(PIC1DP_ERR_ARG, "%s", err.c_str());
  return reset_derived_state(c);
}

int pic1dp_hip_checkpoint_read(pic1dp_ctx *c, const char *path) {
  CHECK_CTX(c);
  std::string err;
  ckpt::Reader r;
  if (r.open(path, &err)) return fail(PIC1DP_ERR_ARG, "%s", err.c_str());
  const ckpt::Small &f = r.small();
  char buf[128];
  if (const char *what = first_difference(c, f, buf, sizeof buf))
    return fail(PIC1DP_ERR_ARG, "checkpoint_read: %s was written by a run that differs from this context in: %s", path, what);
  if (f.rng_ready && f.rng_words != Multirand::state_words())
    return fail(PIC1DP_ERR_ARG, "checkpoint_read: generators of %d state words, this library's have %d", f.rng_words, Multirand::state_words());
  if (c->charge_pending) return fail(PIC1DP_ERR_STATE, "checkpoint_read: charge_local is waiting for charge_reduced");
  std::vector<Multirand> rng(c->blk_rng.size());
  if (f.rng_ready)
    for (int b = 0; b < c->plan.nblk; ++b)
      if (!rng[b].import_state(f.rng[b].engine, f.rng[b].pos, f.rng[b].held, f.rng[b].val, f.rng[b].q))
        return fail(PIC1DP_ERR_ARG, "checkpoint_read: block %d's generator state is not one of this library's generators", b);
  // ---- from here on the context changes: unloaded until everything has arrived and the digests agree ----
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->st));
  c->loaded = false;
  if (int rc = reset_derived_state(c)) return rc;
  const int ns = c->in.nspecies;
  const size_t nx = c->in.nx, nm = c->in.nmode;
  double *h = nullptr;
  if (int rc = pinned(c, static_cast<size_t>(kChunkDoubles), &h)) return rc;
  c->cur = 0;  // (the file's markers go to set 0, where the tail slots live)
  for (int s = 0; s < ns; ++s) {
    Species &S = c->sp[s];
    double *dst[4] = {S.set[0].x, S.set[0].v, S.set[0].w, S.p};
    for (int k = 0; k < 4; ++k)
      for (int64_t off = 0; off < S.nalloc; off += kChunkDoubles) {
        const int64_t n = std::min(kChunkDoubles, S.nalloc - off);
        if (r.markers(s, k, off, h, n, &err)) return fail(PIC1DP_ERR_ARG, "%s", err.c_str());
        if (int rc = put_range(c, dst[k], off, h, n)) return rc;
      }
    S.np = f.np[s];
    c->blk_np[s] = f.blk_np[s];
    HIP_TRY(hipMemcpy(S.fxb, &f.fxb[4 * static_cast<size_t>(s)], 32, hipMemcpyHostToDevice));
    c->diag[s].max_p = f.max_p[s], c->diag[s].max_w = f.max_w[s], c->diag[s].fixed = f.fixed[s] != 0;
  }
  HIP_TRY(hipMemcpy(c->d_E, f.E.data(), 8 * nx, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->d_chargeden, f.cd.data(), 8 * nx, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->d_mode_re, f.re.data(), 8 * nm, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->d_mode_im, f.im.data(), 8 * nm, hipMemcpyHostToDevice));
  c->hist_count = static_cast<int64_t>(f.hist.size());
  if (c->hist_count > 0) HIP_TRY(hipMemcpy(c->d_hist, f.hist.data(), 8 * f.hist.size(), hipMemcpyHostToDevice));
  c->imerge = f.imerge, c->iremove = f.iremove, c->isplit = f.isplit;
  c->rng_ready = f.rng_ready != 0;
  if (c->rng_ready) c->blk_rng = rng;
  c->itime = f.itime, c->time = f.time;
  uint64_t got[PIC1DP_MAX_SPECIES][4];
  if (int rc = device_digests(c, &got[0][0])) return rc;
  for (int s = 0; s < ns; ++s)
    for (int k = 0; k < 4; ++k)
      if (got[s][k] != f.digest[s][k])
        return fail(PIC1DP_ERR_ARG, "checkpoint_read: digest mismatch in the markers of species %d, array %s: %016llx on the device, %016llx in "
                    "the file; the context is left without markers", s, ckpt::kArrayNames[k], (unsigned long long)got[s][k],
                    (unsigned long long)f.digest[s][k]);
  c->loaded = true;
  return reset_derived_state(c);
}

int pic1dp_hip_checkpoint_info(const char *path, pic1dp_input *in, pic1dp_checkpoint_info *info) {
  std::string err;
  ckpt::Reader r;
  if (r.open(path, &err)) return fail(PIC1DP_ERR_ARG, "%s", err.c_str());
  const ckpt::Small &f = r.small();
  if (in) *in = f.in;
  if (info) {
    std::memset(info, 0, sizeof *info);
    info->format_version = static_cast<int32_t>(ckpt::kVersion);
    info->nspecies = f.in.nspecies;
    info->file_bytes = static_cast<int64_t>(r.geo().total);
    info->input_size = static_cast<int64_t>(sizeof(pic1dp_input));
    info->layout.rank = f.rank, info->layout.nranks = f.nranks, info->layout.npe = f.npe, info->layout.device = -1;
    for (int k = 0; k < ckpt::kNumSettings; ++k) info->settings[k] = f.settings[k];
    info->itime = f.itime, info->time = f.time;
    info->nblk = f.nblk;
    info->imerge = f.imerge, info->iremove = f.iremove, info->isplit = f.isplit, info->rng_ready = f.rng_ready;
    info->hist_count = static_cast<int64_t>(f.hist.size());
    for (int s = 0; s < f.in.nspecies; ++s) {
      info->nalloc[s] = f.nalloc[s], info->np[s] = f.np[s];
      for (int k = 0; k < 4; ++k) info->digest[s][k] = f.digest[s][k];
    }
    info->checksum = r.checksum();
  }
  return 0;
}

int pic1dp_hip_checkpoint_verify(const char *path) {
  std::string err;
  ckpt::Reader r;
  if (r.open(path, &err)) return fail(PIC1DP_ERR_ARG, "%s", err.c_str());
  if (r.verify_markers(&err)) return fail(PIC1DP_ERR_ARG, "%s", err.c_str());
  return 0;
}

}  // extern "C"
