// checkpoint_check.cpp -- a stand-alone host program (tests/test_checkpoint_host.py builds it with
// -fsanitize=address,undefined together with checkpoint.cpp, and runs it): the checkpoint file's Writer and Reader
// (pic1dp_amd/csrc/checkpoint.hpp) write, read and verify a small file of two species, and the reader is fed malformed
// files -- wrong magic, another version, truncated, too long, flipped bits, another input size, counts that lie.
// usage: checkpoint_check <directory to write in>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../pic1dp_amd/csrc/checkpoint.hpp"

using namespace pic1dp;

namespace {

int checks = 0, failed = 0;
void expect(bool ok, const char *what, const std::string &detail = "") {
  ++checks;
  if (!ok) {
    ++failed;
    std::printf("FAILED: %s %s\n", what, detail.c_str());
  }
}

uint64_t lcg(uint64_t &s) { return s = s * 6364136223846793005ull + 1442695040888963407ull; }

std::vector<unsigned char> slurp(const std::string &p) {
  std::vector<unsigned char> b;
  if (std::FILE *f = std::fopen(p.c_str(), "rb")) {
    unsigned char buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    std::fclose(f);
  }
  return b;
}
void spit(const std::string &p, const std::vector<unsigned char> &b) {
  std::FILE *f = std::fopen(p.c_str(), "wb");
  if (f) {
    std::fwrite(b.data(), 1, b.size(), f);
    std::fclose(f);
  }
}

// open (and verify) must fail with `word` in the message
void refused(const std::string &p, const std::vector<unsigned char> &b, const char *word, bool by_open = true) {
  spit(p, b);
  ckpt::Reader r;
  std::string err;
  int rc = r.open(p.c_str(), &err);
  if (by_open) {
    expect(rc == PIC1DP_ERR_ARG && err.find(word) != std::string::npos, word, err);
    return;
  }
  expect(rc == 0, "open before verify", err);
  if (rc == 0) {
    rc = r.verify_markers(&err);
    expect(rc == PIC1DP_ERR_ARG && err.find(word) != std::string::npos, word, err);
  }
}

}  // namespace

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const std::string path = dir + "/check.ckpt", bad = dir + "/bad.ckpt";
  uint64_t seed = 12345;
  ckpt::Small s;
  std::memset(&s.in, 0, sizeof s.in);
  s.in.abi_version = PIC1DP_ABI_VERSION, s.in.nspecies = 2, s.in.nx = 12, s.in.nmode = 3;
  s.nblk = 2, s.npe = 2, s.rng_words = 7, s.rng_ready = 1;
  s.itime = 9, s.time = 0.9;
  s.imerge = 1, s.iremove = 0, s.isplit = 2;
  for (int k = 0; k < ckpt::kNumSettings; ++k) s.settings[k] = k;
  s.nalloc = {5000, 131}, s.np = {4097, 131};
  s.blk_np = {{2048, 2049}, {65, 66}};
  auto fill = [&](std::vector<double> &v, size_t n) {
    v.resize(n);
    for (double &x : v) x = static_cast<double>(static_cast<int64_t>(lcg(seed) >> 11)) * 0x1p-40;
  };
  fill(s.E, 12), fill(s.cd, 12), fill(s.re, 3), fill(s.im, 3), fill(s.hist, 9);
  fill(s.max_p, 2), fill(s.max_w, 2);
  s.fixed = {1, 0};
  s.fxb.resize(8);
  for (uint64_t &w : s.fxb) w = lcg(seed);
  s.rng.resize(2);
  for (ckpt::RngState &r : s.rng) {
    r.engine = 3, r.pos = 4, r.held = 1, r.val = -0.5;
    r.q.resize(7);
    for (uint64_t &w : r.q) w = lcg(seed);
  }
  std::vector<std::vector<double>> m(8);
  for (int sp = 0; sp < 2; ++sp)
    for (int k = 0; k < 4; ++k) {
      fill(m[4 * sp + k], static_cast<size_t>(s.nalloc[sp]));
      s.digest[sp][k] = digest_words(reinterpret_cast<const uint64_t *>(m[4 * sp + k].data()), s.nalloc[sp]);
    }

  std::string err;
  {
    ckpt::Writer w;
    expect(w.begin(path.c_str(), s, &err) == 0, "begin", err);
    for (int i = 0; i < 8; ++i) {  // in uneven pieces
      const int64_t n = static_cast<int64_t>(m[i].size()), cut = n / 3;
      expect(w.markers(m[i].data(), cut, &err) == 0, "markers", err);
      expect(w.markers(m[i].data() + cut, n - cut, &err) == 0, "markers", err);
    }
    expect(slurp(path).empty(), "the file does not carry its name before it is complete");
    expect(w.finish(s, &err) == 0, "finish", err);
  }
  {  // an abandoned write leaves nothing
    ckpt::Writer w;
    expect(w.begin(bad.c_str(), s, &err) == 0, "begin", err);
  }
  expect(slurp(bad).empty() && slurp(bad + ".tmp").empty(), "an abandoned write leaves no file");
  {  // too many markers are refused
    ckpt::Writer w;
    expect(w.begin(bad.c_str(), s, &err) == 0, "begin", err);
    std::vector<double> big(30000, 1.0);
    expect(w.markers(big.data(), 30000, &err) != 0, "more marker data than the sections hold");
  }
  {
    ckpt::Reader r;
    expect(r.open(path.c_str(), &err) == 0, "open", err);
    const ckpt::Small &g = r.small();
    expect(std::memcmp(&g.in, &s.in, sizeof s.in) == 0 && g.nblk == 2 && g.npe == 2 && g.itime == 9 && g.time == 0.9 && g.isplit == 2,
           "section A comes back");
    expect(g.nalloc == s.nalloc && g.np == s.np && g.blk_np == s.blk_np, "sizes come back");
    expect(g.E == s.E && g.cd == s.cd && g.re == s.re && g.im == s.im && g.hist == s.hist, "fields and history come back");
    expect(g.fxb == s.fxb && g.max_p == s.max_p && g.max_w == s.max_w && g.fixed == s.fixed, "bounds come back");
    expect(g.rng.size() == 2 && g.rng[1].q == s.rng[1].q && g.rng[0].pos == 4 && g.rng[0].val == -0.5, "generators come back");
    expect(std::memcmp(g.digest, s.digest, sizeof s.digest) == 0, "digests come back");
    std::vector<double> buf(131);
    expect(r.markers(1, 2, 0, buf.data(), 131, &err) == 0 && buf == m[6], "a marker section comes back", err);
    expect(r.markers(0, 3, 4990, buf.data(), 10, &err) == 0 && std::memcmp(buf.data(), m[3].data() + 4990, 80) == 0, "... and a piece of one");
    expect(r.markers(0, 3, 4990, buf.data(), 11, &err) != 0, "a range beyond the section is refused");
    expect(r.verify_markers(&err) == 0, "verify", err);
  }
  const std::vector<unsigned char> good = slurp(path);
  ckpt::Geometry geo;
  expect(ckpt::geometry(s, &geo, &err) && geo.total == good.size(), "geometry");
  std::vector<unsigned char> b = good;
  b[3] ^= 0x20;
  refused(bad, b, "magic");
  b = good, b[8] += 1;
  refused(bad, b, "version 2");
  b = good, b.pop_back();
  refused(bad, b, "truncated");
  b.assign(good.begin(), good.begin() + static_cast<long>(geo.tail_off));
  refused(bad, b, "truncated");
  b.assign(good.begin(), good.begin() + 40);
  refused(bad, b, "truncated");
  b = good, b.push_back(0);
  refused(bad, b, "1 more");
  b = good, b[24] += 8;
  refused(bad, b, "input struct");
  b = good, b[geo.marker_off[1][2] + 77] ^= 0x04;
  refused(bad, b, "species 1, array w", false);
  b = good, b[geo.marker_off[0][0]] ^= 0x80;
  refused(bad, b, "species 0, array x", false);
  for (uint64_t off : {geo.tail_off + 5, geo.tail_off + 8 * 30 + 1, geo.tail_off + 8 * 45, geo.total - 1, static_cast<uint64_t>(70), geo.head_bytes - 3}) {
    b = good, b[off] ^= 0x01;
    refused(bad, b, "checksum");
  }
  // counts that lie, with header lengths that follow them: refused before anything is allocated or read out of bounds
  const size_t a0 = ckpt::kHeaderBytes + ((sizeof(pic1dp_input) + 7) & ~static_cast<size_t>(7));
  b = good, b[a0 + 12] = 0xff, b[a0 + 13] = 0xff, b[a0 + 14] = 0xff, b[a0 + 15] = 0x7f;   // nblk = 2^31 - 1
  refused(bad, b, "out of range");
  b = good, std::memset(&b[a0 + 88], 0xff, 7);                                               // nalloc of species 0: huge
  refused(bad, b, "");
  b = good, b[40] += 8;                                                                      // header + A longer than they are
  refused(bad, b, "");
  std::remove(path.c_str());
  std::remove(bad.c_str());
  std::printf("%d checks, %d failed\n", checks, failed);
  return failed ? 1 : 0;
}
