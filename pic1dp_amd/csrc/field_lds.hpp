// field_lds.hpp -- the dynamic LDS of the one-workgroup field kernels (kernels_field.hip), laid out ONCE per kernel family:
// the kernel takes its pointers from the struct and its launcher the byte count from the same struct, so a region added to
// one is in the other.  Plain arithmetic for host and device, no HIP call; tests/test_field_lds_host.py pins every byte and
// thread count on the host (include/pic1dp_probe.h).  Offsets are in doubles from the start of the dynamic LDS.
#pragma once
#include "kernels.hpp"

namespace pic1dp {

constexpr int FIELD_THREADS = 256;

// k_field_solve and its _pred, _pred_sums, _xchg siblings; k_field_solve_pair<SRC>
struct SolveLds {
  size_t cd;    // [nx] chargeden
  size_t mode;  // [2 nmode] re then im
  size_t scr;   // [16] block_sum's scratch
  size_t tab;   // [2][nmode][nx] the products of the tables, where they fit (FieldArgs::tab_lds)
  size_t vec;   // k_field_solve_pair<1>: [charge2 | Z-weighted prediction slices] of this rank, then of all ranks
  size_t end;
  __host__ __device__ SolveLds(int nx, int nmode, bool tab_lds, size_t vec_doubles = 0)
      : cd(0), mode(cd + nx), scr(mode + 2 * nmode), tab(scr + 16),
        vec(tab + (tab_lds ? 2 * static_cast<size_t>(nmode) * nx : 0)), end(vec + vec_doubles) {}
  __host__ __device__ static SolveLds pair(int nx, int nmode, bool tab_lds, bool xchg) {
    return SolveLds(nx, nmode, tab_lds, xchg ? pack_doubles(nx, nmode, 1) : 0);
  }
  __host__ __device__ size_t bytes() const { return sizeof(double) * end; }
};

// the lean pair kernels of ONE kept mode: k_field_solve_pair1<SRC> (wave partials of its six sums) and
// k_field_solve_pair_sums1<SRC>.  Both product rows start on 16 bytes (chain_sum_lds reads them in pairs).
struct LeanPairLds {
  size_t pc;    // [ne] fre * chargeden, ne = nx rounded up to even
  size_t ps;    // [ne] fim * chargeden
  size_t w;     // pair1: [FIELD_THREADS / 64][6] wave partials of the six sums
  size_t mode;  // [8] re, im, then the six sums of the workgroup
  size_t scr;   // [16] block_sum's scratch
  size_t part;  // [2 npe, rounded up to even] partial chains of the npe-rank order
  size_t vec;   // SRC 1: this rank's packed vector, then the sum over ranks
  size_t end;
  __host__ __device__ LeanPairLds(int nx, int npe, bool wave_partials, size_t vec_doubles)
      : pc(0), ps(pc + ((static_cast<size_t>(nx) + 1) & ~static_cast<size_t>(1))), w(ps + (ps - pc)),
        mode(w + (wave_partials ? (FIELD_THREADS / 64) * 6 : 0)), scr(mode + 8), part(scr + 16),
        vec(part + ((2 * static_cast<size_t>(npe) + 1) & ~static_cast<size_t>(1))), end(vec + vec_doubles) {}
  // xchg (SRC 1): [charge2 | R0 | RA | RB]
  __host__ __device__ static LeanPairLds pair1(int nx, int npe, bool xchg) {
    return LeanPairLds(nx, npe, true, xchg ? pack_doubles(nx, 1, 1) : 0);
  }
  // xchg (SRC 1): [charge2 | six sums | pad]
  __host__ __device__ static LeanPairLds sums1(int nx, int npe, bool xchg) {
    return LeanPairLds(nx, npe, false, xchg ? pack_doubles(nx, 1, 2) : 0);
  }
  __host__ __device__ size_t bytes() const { return sizeof(double) * end; }
};

// which kernel launch_field_solve_pair runs, with how many threads and how much dynamic LDS
enum FieldFamily { FIELD_SOLVE = 0, FIELD_PAIR = 1, FIELD_PAIR1 = 2, FIELD_PAIR_SUMS1 = 3 };
struct FieldLaunch {
  FieldFamily family;
  int threads;
  size_t bytes;
};
inline FieldLaunch solve_launch(int nx, int nmode, bool tab_lds) {
  return {FIELD_SOLVE, FIELD_THREADS, SolveLds(nx, nmode, tab_lds).bytes()};
}
inline FieldLaunch pair_launch(int nx, int nmode, int npe, bool tab_lds, bool xchg, int pred_kind) {
  if (pred_kind == 2)  // the six sums of ONE kept mode: as many threads as the grid has cells, up to 1024 (four cells each)
    return {FIELD_PAIR_SUMS1, nx > 2048 ? 1024 : (nx > 1024 ? 512 : FIELD_THREADS), LeanPairLds::sums1(nx, npe, xchg).bytes()};
  if (nmode == 1 && tab_lds)  // the lean kernel of the usual case
    return {FIELD_PAIR1, FIELD_THREADS, LeanPairLds::pair1(nx, npe, xchg).bytes()};
  return {FIELD_PAIR, FIELD_THREADS, SolveLds::pair(nx, nmode, tab_lds, xchg).bytes()};
}

}  // namespace pic1dp
