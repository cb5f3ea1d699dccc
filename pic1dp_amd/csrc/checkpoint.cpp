// checkpoint.cpp -- writer and reader of the checkpoint file (checkpoint.hpp; the format: INTEGRATION.md section 7).
#include "checkpoint.hpp"

#include <algorithm>
#include <cerrno>
#include <cstdarg>
#include <cstring>

namespace pic1dp {
namespace ckpt {

const char *const kSettingNames[kNumSettings] = {"charge_sum",  "diag_sum",    "field_transform", "field_solver",
                                                 "step_mode",   "fuse_output", "seed_offset"};
const char *const kArrayNames[4] = {"x", "v", "w", "p"};

namespace {

int bad(std::string *err, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (err) *err = buf;
  return PIC1DP_ERR_ARG;
}

constexpr size_t pad8(size_t n) { return (n + 7) & ~static_cast<size_t>(7); }
constexpr size_t kInputBytes = pad8(sizeof(pic1dp_input));

struct Out {
  std::vector<unsigned char> b;
  void raw(const void *p, size_t n) {
    const unsigned char *q = static_cast<const unsigned char *>(p);
    b.insert(b.end(), q, q + n);
  }
  void i32(int32_t v) { raw(&v, 4); }
  void u32(uint32_t v) { raw(&v, 4); }
  void i64(int64_t v) { raw(&v, 8); }
  void u64(uint64_t v) { raw(&v, 8); }
  void f64(double v) { raw(&v, 8); }
  void pad() { b.resize(pad8(b.size()), 0); }
};

struct In {
  const unsigned char *p;
  size_t n, at = 0;
  bool ok = true;
  void raw(void *d, size_t k) {
    if (!ok || k > n - at) {
      ok = false;
      std::memset(d, 0, k);
      return;
    }
    std::memcpy(d, p + at, k);
    at += k;
  }
  int32_t i32() { int32_t v; raw(&v, 4); return v; }
  uint32_t u32() { uint32_t v; raw(&v, 4); return v; }
  int64_t i64() { int64_t v; raw(&v, 8); return v; }
  uint64_t u64() { uint64_t v; raw(&v, 8); return v; }
  double f64() { double v; raw(&v, 8); return v; }
  void skip_to8() {
    if (pad8(at) <= n)
      at = pad8(at);
    else
      ok = false;
  }
};

uint64_t words_sum(const std::vector<unsigned char> &b, int64_t i0) {
  // (the buffers are whole 8-byte words; copied out so that no unaligned word is ever read)
  uint64_t s = 0, g = static_cast<uint64_t>(i0 + 1) * DIGEST_GOLD;
  for (size_t o = 0; o + 8 <= b.size(); o += 8, g += DIGEST_GOLD) {
    uint64_t w;
    std::memcpy(&w, b.data() + o, 8);
    s += digest_mix(w, g);
  }
  return s;
}

// header (checksum word zero) and section A
void build_head(const Small &s, const Geometry &g, Out *o) {
  o->raw(kMagic, 8);
  o->u32(kVersion);
  o->u32(kEndianTag);
  o->u64(g.total);
  o->u64(sizeof(pic1dp_input));
  o->u64(0);  // the checksum's place (offset 32)
  o->u64(g.head_bytes);
  o->u64(g.tail_bytes);
  o->u64(0);
  o->raw(&s.in, sizeof(pic1dp_input));
  o->pad();
  o->i32(s.rank), o->i32(s.nranks), o->i32(s.npe), o->i32(s.nblk);
  for (int k = 0; k < kNumSettings; ++k) o->i32(s.settings[k]);
  o->i32(s.rng_words);
  o->i32(s.itime), o->i32(s.rng_ready);
  o->f64(s.time);
  o->i32(s.imerge), o->i32(s.iremove), o->i32(s.isplit), o->i32(0);
  o->i64(static_cast<int64_t>(s.hist.size()));
  for (int sp = 0; sp < s.in.nspecies; ++sp) {
    o->i64(s.nalloc[sp]), o->i64(s.np[sp]);
    for (int b = 0; b < s.nblk; ++b) o->i64(s.blk_np[sp][b]);
  }
}

void build_tail(const Small &s, Out *o) {
  o->raw(s.E.data(), 8 * s.E.size()), o->raw(s.cd.data(), 8 * s.cd.size());
  o->raw(s.re.data(), 8 * s.re.size()), o->raw(s.im.data(), 8 * s.im.size());
  o->raw(s.hist.data(), 8 * s.hist.size());
  if (s.rng_words > 0)
    for (int b = 0; b < s.nblk; ++b) {
      const RngState &r = s.rng[b];
      o->i32(r.engine), o->i32(r.pos), o->i32(r.held), o->i32(0);
      o->f64(r.val);
      o->raw(r.q.data(), 8 * r.q.size());
    }
  o->raw(s.fxb.data(), 8 * s.fxb.size());
  for (int sp = 0; sp < s.in.nspecies; ++sp) o->f64(s.max_p[sp]), o->f64(s.max_w[sp]), o->i32(s.fixed[sp]), o->i32(0);
  for (int sp = 0; sp < s.in.nspecies; ++sp)
    for (int k = 0; k < 4; ++k) o->u64(s.digest[sp][k]);
}

// the vectors of s have the sizes its counts ask for
bool shaped(const Small &s, size_t nhist, std::string *err) {
  const size_t ns = static_cast<size_t>(s.in.nspecies), nx = static_cast<size_t>(s.in.nx), nm = static_cast<size_t>(s.in.nmode);
  bool ok = s.nalloc.size() == ns && s.np.size() == ns && s.blk_np.size() == ns && s.E.size() == nx && s.cd.size() == nx &&
            s.re.size() == nm && s.im.size() == nm && s.hist.size() == nhist && s.fxb.size() == 4 * ns && s.max_p.size() == ns &&
            s.max_w.size() == ns && s.fixed.size() == ns &&
            s.rng.size() == (s.rng_words > 0 ? static_cast<size_t>(s.nblk) : static_cast<size_t>(0));
  for (size_t sp = 0; ok && sp < ns; ++sp) ok = s.blk_np[sp].size() == static_cast<size_t>(s.nblk);
  for (size_t b = 0; ok && b < s.rng.size(); ++b) ok = s.rng[b].q.size() == static_cast<size_t>(s.rng_words);
  if (!ok) bad(err, "checkpoint: a section's size does not match the counts");
  return ok;
}

}  // namespace

bool geometry(const Small &s, Geometry *g, std::string *err) {
  const pic1dp_input &in = s.in;
  if (in.nspecies < 1 || in.nspecies > PIC1DP_MAX_SPECIES) return bad(err, "checkpoint: nspecies %d out of range", in.nspecies), false;
  if (in.nx < 1 || in.nx > (1 << 24)) return bad(err, "checkpoint: nx %d out of range", in.nx), false;
  if (in.nmode < 1 || in.nmode > PIC1DP_MAX_MODES) return bad(err, "checkpoint: nmode %d out of range", in.nmode), false;
  if (s.nblk < 1 || s.nblk > (1 << 20)) return bad(err, "checkpoint: %d blocks out of range", s.nblk), false;
  if (s.rng_words < 0 || s.rng_words > (1 << 20)) return bad(err, "checkpoint: %d generator words out of range", s.rng_words), false;
  const int64_t nhist = static_cast<int64_t>(s.hist.size());
  if (nhist > kMaxHistory) return bad(err, "checkpoint: an energy history of %lld entries is out of range", (long long)nhist), false;
  if (s.nalloc.size() != static_cast<size_t>(in.nspecies) || s.np.size() != s.nalloc.size())
    return bad(err, "checkpoint: a section's size does not match the counts"), false;
  const uint64_t ns = static_cast<uint64_t>(in.nspecies), nblk = static_cast<uint64_t>(s.nblk);
  g->head_bytes = kHeaderBytes + kInputBytes + 16 + 32 + 16 + 16 + 8 + ns * (16 + 8 * nblk);
  uint64_t at = g->head_bytes;
  for (int sp = 0; sp < in.nspecies; ++sp) {
    const int64_t n = s.nalloc[sp];
    if (n < 0 || n > (static_cast<int64_t>(1) << 40)) return bad(err, "checkpoint: species %d: %lld slots out of range", sp, (long long)n), false;
    if (s.np[sp] < 0 || s.np[sp] > n) return bad(err, "checkpoint: species %d: np %lld beyond its %lld slots", sp, (long long)s.np[sp], (long long)n), false;
    for (int k = 0; k < 4; ++k) {
      g->marker_off[sp][k] = at;
      at += 8 * static_cast<uint64_t>(n);
    }
  }
  g->tail_off = at;
  g->tail_bytes = 8 * (2 * static_cast<uint64_t>(in.nx) + 2 * static_cast<uint64_t>(in.nmode) + static_cast<uint64_t>(nhist)) +
                  (s.rng_words > 0 ? nblk * (24 + 8 * static_cast<uint64_t>(s.rng_words)) : 0) + ns * 32 + ns * 24 + ns * 32;
  g->total = at + g->tail_bytes;
  return true;
}

// ---------------------------------------------------------------------------
int Writer::begin(const char *path, const Small &s, std::string *err) {
  abandon();
  if (!path || !*path) return bad(err, "checkpoint: no file name");
  if (!geometry(s, &g_, err) || !shaped(s, s.hist.size(), err)) return PIC1DP_ERR_ARG;
  Out o;
  build_head(s, g_, &o);
  if (o.b.size() != g_.head_bytes) return bad(err, "internal: checkpoint head of %zu bytes, %llu planned", o.b.size(), (unsigned long long)g_.head_bytes);
  head_.swap(o.b);
  path_ = path;
  tmp_ = path_ + ".tmp";
  f_ = std::fopen(tmp_.c_str(), "wb");
  if (!f_) return bad(err, "checkpoint: cannot create %s: %s", tmp_.c_str(), std::strerror(errno));
  done_ = 0;
  if (std::fwrite(head_.data(), 1, head_.size(), f_) != head_.size()) {
    abandon();
    return bad(err, "checkpoint: writing %s failed", tmp_.c_str());
  }
  return 0;
}

int Writer::markers(const double *a, int64_t n, std::string *err) {
  if (!f_) return bad(err, "checkpoint: no file open");
  if (n <= 0) return 0;
  if (done_ + 8 * static_cast<uint64_t>(n) > g_.tail_off - g_.head_bytes) {
    abandon();
    return bad(err, "internal: more marker data than the checkpoint's sections hold");
  }
  if (std::fwrite(a, 8, static_cast<size_t>(n), f_) != static_cast<size_t>(n)) {
    abandon();
    return bad(err, "checkpoint: writing %s failed: %s", tmp_.c_str(), std::strerror(errno));
  }
  done_ += 8 * static_cast<uint64_t>(n);
  return 0;
}

int Writer::finish(const Small &s, std::string *err) {
  if (!f_) return bad(err, "checkpoint: no file open");
  Geometry g;
  if (!geometry(s, &g, err) || !shaped(s, s.hist.size(), err)) {
    abandon();
    return PIC1DP_ERR_ARG;
  }
  if (g.total != g_.total || done_ != g_.tail_off - g_.head_bytes) {
    abandon();
    return bad(err, "internal: the checkpoint's marker sections are incomplete");
  }
  Out t;
  build_tail(s, &t);
  if (t.b.size() != g_.tail_bytes) {
    abandon();
    return bad(err, "internal: checkpoint tail of %zu bytes, %llu planned", t.b.size(), (unsigned long long)g_.tail_bytes);
  }
  const uint64_t sum = words_sum(head_, 0) + words_sum(t.b, static_cast<int64_t>(head_.size() / 8));
  bool ok = std::fwrite(t.b.data(), 1, t.b.size(), f_) == t.b.size();
  ok = ok && std::fseek(f_, 32, SEEK_SET) == 0 && std::fwrite(&sum, 8, 1, f_) == 1;
  ok = ok && std::fflush(f_) == 0;
  ok = (std::fclose(f_) == 0) && ok;
  f_ = nullptr;
  if (!ok || std::rename(tmp_.c_str(), path_.c_str()) != 0) {
    std::remove(tmp_.c_str());
    return bad(err, "checkpoint: writing %s failed: %s", path_.c_str(), std::strerror(errno));
  }
  return 0;
}

void Writer::abandon() {
  if (f_) {
    std::fclose(f_);
    f_ = nullptr;
    std::remove(tmp_.c_str());
  }
}

// ---------------------------------------------------------------------------
void Reader::close() {
  if (f_) std::fclose(f_);
  f_ = nullptr;
}

int Reader::open(const char *path, std::string *err) {
  close();
  s_ = Small{};
  if (!path || !*path) return bad(err, "checkpoint: no file name");
  f_ = std::fopen(path, "rb");
  if (!f_) return bad(err, "checkpoint: cannot open %s: %s", path, std::strerror(errno));
  auto fail_close = [&](int rc) {
    close();
    return rc;
  };
  if (std::fseek(f_, 0, SEEK_END) != 0) return fail_close(bad(err, "checkpoint: cannot seek in %s", path));
  const long long fsize = static_cast<long long>(ftello(f_));
  std::rewind(f_);
  unsigned char hdr[kHeaderBytes];
  if (fsize < static_cast<long long>(kHeaderBytes) || std::fread(hdr, 1, kHeaderBytes, f_) != kHeaderBytes)
    return fail_close(bad(err, "checkpoint: %s is truncated: %lld bytes, less than a header", path, fsize));
  if (std::memcmp(hdr, kMagic, 8) != 0) return fail_close(bad(err, "checkpoint: wrong magic: %s is not a pic1dp checkpoint", path));
  In h{hdr, kHeaderBytes};
  h.at = 8;
  const uint32_t version = h.u32(), endian = h.u32();
  const uint64_t total = h.u64(), insize = h.u64(), checksum = h.u64(), head_bytes = h.u64(), tail_bytes = h.u64();
  if (endian != kEndianTag) return fail_close(bad(err, "checkpoint: byte order tag %08x: the file is not little-endian", endian));
  if (version != kVersion) return fail_close(bad(err, "checkpoint: format version %u, this library reads version %u", version, kVersion));
  if (insize != sizeof(pic1dp_input))
    return fail_close(bad(err, "checkpoint: input struct of %llu bytes, this library's has %zu", (unsigned long long)insize, sizeof(pic1dp_input)));
  if (static_cast<unsigned long long>(fsize) < total)
    return fail_close(bad(err, "checkpoint: %s is truncated: %lld bytes, the header says %llu", path, fsize, (unsigned long long)total));
  if (static_cast<unsigned long long>(fsize) > total)
    return fail_close(bad(err, "checkpoint: %s has %lld bytes, %llu more than the header's length", path, fsize,
                          (unsigned long long)(fsize - total)));
  const uint64_t min_head = kHeaderBytes + kInputBytes + 88;
  if (head_bytes < min_head || head_bytes > total || head_bytes % 8 != 0 || tail_bytes > total - head_bytes || tail_bytes % 8 != 0 ||
      head_bytes > (static_cast<uint64_t>(1) << 32) || tail_bytes > (static_cast<uint64_t>(1) << 40))
    return fail_close(bad(err, "checkpoint: section lengths in the header are inconsistent"));
  std::vector<unsigned char> head(static_cast<size_t>(head_bytes));
  std::rewind(f_);
  if (std::fread(head.data(), 1, head.size(), f_) != head.size()) return fail_close(bad(err, "checkpoint: reading %s failed", path));
  In a{head.data(), head.size()};
  a.at = kHeaderBytes;
  a.raw(&s_.in, sizeof(pic1dp_input));
  a.skip_to8();
  s_.rank = a.i32(), s_.nranks = a.i32(), s_.npe = a.i32(), s_.nblk = a.i32();
  for (int k = 0; k < kNumSettings; ++k) s_.settings[k] = a.i32();
  s_.rng_words = a.i32();
  s_.itime = a.i32(), s_.rng_ready = a.i32();
  s_.time = a.f64();
  s_.imerge = a.i32(), s_.iremove = a.i32(), s_.isplit = a.i32();
  (void)a.i32();
  const int64_t nhist = a.i64();
  const pic1dp_input &in = s_.in;
  if (!a.ok || in.nspecies < 1 || in.nspecies > PIC1DP_MAX_SPECIES || s_.nblk < 1 || s_.nblk > (1 << 20) || nhist < 0 || nhist > kMaxHistory)
    return fail_close(bad(err, "checkpoint: counts in section A are out of range (nspecies %d, blocks %d, history %lld)", in.nspecies,
                          s_.nblk, (long long)nhist));
  if (head_bytes != min_head + static_cast<uint64_t>(in.nspecies) * (16 + 8 * static_cast<uint64_t>(s_.nblk)))
    return fail_close(bad(err, "checkpoint: section A has %llu bytes, its counts ask for another length", (unsigned long long)head_bytes));
  s_.nalloc.resize(in.nspecies), s_.np.resize(in.nspecies), s_.blk_np.resize(in.nspecies);
  for (int sp = 0; sp < in.nspecies; ++sp) {
    s_.nalloc[sp] = a.i64(), s_.np[sp] = a.i64();
    s_.blk_np[sp].resize(s_.nblk);
    for (int b = 0; b < s_.nblk; ++b) s_.blk_np[sp][b] = a.i64();
  }
  s_.hist.resize(static_cast<size_t>(nhist));
  if (!a.ok) return fail_close(bad(err, "checkpoint: section A is malformed"));
  if (!geometry(s_, &g_, err)) return fail_close(PIC1DP_ERR_ARG);
  if (g_.head_bytes != head_bytes || g_.tail_bytes != tail_bytes || g_.total != total)
    return fail_close(bad(err, "checkpoint: the sections add up to %llu bytes, the header says %llu: a section is missing or truncated",
                          (unsigned long long)g_.total, (unsigned long long)total));
  std::vector<unsigned char> tail(static_cast<size_t>(tail_bytes));
  if (fseeko(f_, static_cast<off_t>(g_.tail_off), SEEK_SET) != 0 || std::fread(tail.data(), 1, tail.size(), f_) != tail.size())
    return fail_close(bad(err, "checkpoint: reading %s failed", path));
  std::memset(head.data() + 32, 0, 8);
  const uint64_t sum = words_sum(head, 0) + words_sum(tail, static_cast<int64_t>(head.size() / 8));
  if (sum != checksum)
    return fail_close(bad(err, "checkpoint: checksum mismatch in the small sections (header, input, settings, counters, fields, energy "
                               "history, generators, bounds or digests): %016llx computed, %016llx in the file",
                          (unsigned long long)sum, (unsigned long long)checksum));
  checksum_ = checksum;
  In t{tail.data(), tail.size()};
  const size_t nx = static_cast<size_t>(in.nx), nm = static_cast<size_t>(in.nmode), ns = static_cast<size_t>(in.nspecies);
  s_.E.resize(nx), s_.cd.resize(nx), s_.re.resize(nm), s_.im.resize(nm);
  t.raw(s_.E.data(), 8 * nx), t.raw(s_.cd.data(), 8 * nx), t.raw(s_.re.data(), 8 * nm), t.raw(s_.im.data(), 8 * nm);
  t.raw(s_.hist.data(), 8 * s_.hist.size());
  if (s_.rng_words > 0) {
    s_.rng.resize(s_.nblk);
    for (RngState &r : s_.rng) {
      r.engine = t.i32(), r.pos = t.i32(), r.held = t.i32();
      (void)t.i32();
      r.val = t.f64();
      r.q.resize(s_.rng_words);
      t.raw(r.q.data(), 8 * r.q.size());
    }
  }
  s_.fxb.resize(4 * ns);
  t.raw(s_.fxb.data(), 8 * s_.fxb.size());
  s_.max_p.resize(ns), s_.max_w.resize(ns), s_.fixed.resize(ns);
  for (size_t sp = 0; sp < ns; ++sp) {
    s_.max_p[sp] = t.f64(), s_.max_w[sp] = t.f64(), s_.fixed[sp] = t.i32();
    (void)t.i32();
  }
  for (size_t sp = 0; sp < ns; ++sp)
    for (int k = 0; k < 4; ++k) s_.digest[sp][k] = t.u64();
  if (!t.ok || t.at != tail.size()) return fail_close(bad(err, "checkpoint: the tail sections are malformed"));
  return 0;
}

int Reader::markers(int s, int k, int64_t off, double *buf, int64_t n, std::string *err) {
  if (!f_) return bad(err, "checkpoint: no file open");
  if (s < 0 || s >= s_.in.nspecies || k < 0 || k > 3 || off < 0 || n < 0 || off + n > s_.nalloc[s])
    return bad(err, "checkpoint: marker range out of bounds");
  if (n == 0) return 0;
  if (fseeko(f_, static_cast<off_t>(g_.marker_off[s][k] + 8 * static_cast<uint64_t>(off)), SEEK_SET) != 0 ||
      std::fread(buf, 8, static_cast<size_t>(n), f_) != static_cast<size_t>(n))
    return bad(err, "checkpoint: reading markers of species %d, array %s failed", s, kArrayNames[k]);
  return 0;
}

int Reader::verify_markers(std::string *err) {
  std::vector<double> buf(static_cast<size_t>(1) << 17);
  static_assert(sizeof(double) == sizeof(uint64_t), "doubles are 64-bit words");
  std::vector<uint64_t> w(buf.size());
  for (int s = 0; s < s_.in.nspecies; ++s)
    for (int k = 0; k < 4; ++k) {
      uint64_t d = 0;
      for (int64_t off = 0; off < s_.nalloc[s]; off += static_cast<int64_t>(buf.size())) {
        const int64_t n = std::min<int64_t>(static_cast<int64_t>(buf.size()), s_.nalloc[s] - off);
        if (int rc = markers(s, k, off, buf.data(), n, err)) return rc;
        std::memcpy(w.data(), buf.data(), 8 * static_cast<size_t>(n));
        d += digest_words(w.data(), n, off);
      }
      if (d != s_.digest[s][k])
        return bad(err, "checkpoint: digest mismatch in the markers of species %d, array %s: %016llx computed, %016llx in the file", s,
                   kArrayNames[k], (unsigned long long)d, (unsigned long long)s_.digest[s][k]);
    }
  return 0;
}

}  // namespace ckpt
}  // namespace pic1dp
