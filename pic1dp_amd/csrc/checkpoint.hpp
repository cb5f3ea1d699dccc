// checkpoint.hpp -- the checkpoint file, host side only: no device, no HIP header.  A file is
//   header (64 B) | section A: input, layout, settings, counters, sizes | the marker sections | the tail: fields, energy
//   history, generators, fixed-point bounds, diagnostics scales, the marker sections' digests
// in 8-byte little-endian words throughout.  The marker sections carry their digests D[s][k] (digest.hpp), everything else
// one checksum: the same mixing over the 8-byte words of header (checksum word taken as zero), section A and tail, in
// file order.  capi_checkpoint.cpp moves the markers between these and the device; tests/checkpoint_check.cpp runs
// Writer and Reader under the host sanitizers.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/pic1dp_hip.h"
#include "digest.hpp"

namespace pic1dp {
namespace ckpt {

constexpr char kMagic[8] = {'P', 'I', 'C', '1', 'D', 'P', 'C', 'K'};
constexpr uint32_t kVersion = 1, kEndianTag = 0x01020304u;
constexpr size_t kHeaderBytes = 64;
constexpr int kNumSettings = 7;
constexpr int64_t kMaxHistory = 1 << 20;  // ctx.hpp kHistCap
// the settings that select arithmetic, in file order
extern const char *const kSettingNames[kNumSettings];
// arrays of a marker section, in file order
extern const char *const kArrayNames[4];

struct RngState {
  int32_t engine = 0, pos = 0, held = 0;
  double val = 0.0;
  std::vector<uint64_t> q;
};

// everything a file holds but the markers
struct Small {
  pic1dp_input in{};
  int32_t rank = 0, nranks = 1, npe = 1, nblk = 1;
  int32_t settings[kNumSettings] = {0, 0, 0, 0, 0, 0, 0};
  int32_t rng_words = 0;          // state words per generator (0: the file carries none)
  int32_t itime = 0, rng_ready = 0;
  double time = 0.0;
  int32_t imerge = 0, iremove = 0, isplit = 0;
  std::vector<int64_t> nalloc, np;            // [nspecies]
  std::vector<std::vector<int64_t>> blk_np;   // [nspecies][nblk]
  std::vector<double> E, cd, re, im, hist;    // [nx], [nx], [nmode], [nmode], [count]
  std::vector<RngState> rng;                  // [nblk] when rng_words > 0
  std::vector<uint64_t> fxb;                  // [nspecies][4]
  std::vector<double> max_p, max_w;           // [nspecies]
  std::vector<int32_t> fixed;                 // [nspecies]
  uint64_t digest[PIC1DP_MAX_SPECIES][4] = {};
};

struct Geometry {
  uint64_t head_bytes = 0;   // header + section A
  uint64_t marker_off[PIC1DP_MAX_SPECIES][4] = {};
  uint64_t tail_off = 0, tail_bytes = 0, total = 0;
};
// false: the sizes in s cannot be a file's (message in *err)
bool geometry(const Small &s, Geometry *g, std::string *err);

// 0, or PIC1DP_ERR_ARG with the cause in *err
class Writer {
 public:
  Writer() = default;
  Writer(const Writer &) = delete;
  Writer &operator=(const Writer &) = delete;
  ~Writer() { abandon(); }
  int begin(const char *path, const Small &s, std::string *err);   // header and section A into path + ".tmp"
  int markers(const double *a, int64_t n, std::string *err);        // the sections' doubles, appended in file order
  int finish(const Small &s, std::string *err);                      // tail, checksum; the file takes its name
  void abandon();                                                    // nothing is left behind
  uint64_t marker_bytes() const { return done_; }

 private:
  std::FILE *f_ = nullptr;
  std::string path_, tmp_;
  std::vector<unsigned char> head_;
  Geometry g_;
  uint64_t done_ = 0;
};

class Reader {
 public:
  Reader() = default;
  Reader(const Reader &) = delete;
  Reader &operator=(const Reader &) = delete;
  ~Reader() { close(); }
  // magic, version, lengths and the checksum verified; everything but the markers parsed
  int open(const char *path, std::string *err);
  const Small &small() const { return s_; }
  const Geometry &geo() const { return g_; }
  uint64_t checksum() const { return checksum_; }
  // doubles [off, off + n) of species s, array k (0 x, 1 v, 2 w, 3 p)
  int markers(int s, int k, int64_t off, double *buf, int64_t n, std::string *err);
  // every marker section against its digest, on the host
  int verify_markers(std::string *err);
  void close();

 private:
  std::FILE *f_ = nullptr;
  Small s_;
  Geometry g_;
  uint64_t checksum_ = 0;
};

}  // namespace ckpt
}  // namespace pic1dp
