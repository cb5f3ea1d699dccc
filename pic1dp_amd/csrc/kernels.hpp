// kernels.hpp -- launch interface of the gfx950 kernels (kernels_step.hip, kernels_push.hip, kernels_field.hip, kernels_diag.hip,
// kernels_moments.hip, ...).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pic1dp_hip.h"
#include "load_seq.hpp"

#include <cstdint>
#include <cstdlib>
#include <type_traits>

// Environment variables.  The product library reads the fifteen of INTEGRATION.md section 6 with std::getenv: switches
// between paths that exist for a functional reason (eager / lazy call sites, two passes / one, tiles / sums, the solve in a
// launch of its own, ...), which the differential tests hold against each other, and operational settings.  Everything a
// MEASUREMENT wants to vary beyond them (launch shapes, thresholds, schedules; tools/ab_*.sh) goes through tuning_env(),
// which only a -DPIC1DP_TUNING build looks at -- `PIC1DP_EXTRA_FLAGS=-DPIC1DP_TUNING PIC1DP_LIB_OUT=.../v_tuning.so python
// pic1dp_amd/build.py --force`, loaded with PIC1DP_LIB; the default build compiles none of it.
#ifdef PIC1DP_TUNING
inline const char *tuning_env(const char *name) { return std::getenv(name); }
#else
inline const char *tuning_env(const char *) { return nullptr; }
#endif
// -DPIC1DP_TRIMS=0 (A/B builds, tools/ab_trims.py): the shared per-marker functions without the result-preserving strength
// reductions of DESIGN.md 2.1 -- the five-operation x / lx always, locate through floor, the charge as a trailing factor
#ifndef PIC1DP_TRIMS
#define PIC1DP_TRIMS 1
#endif
#if defined(PIC1DP_TUNE_STAMPS) && !defined(PIC1DP_TUNING)
#error "-DPIC1DP_TUNE_STAMPS instruments the marker kernels: it belongs to a tuning build (-DPIC1DP_TUNING), never to the product"
#endif

namespace pic1dp {

// Constants of one species' push, pre-formed on the host exactly as the
// reference's compile-time folding would form them (src/pic1dp_input.F90
// parameters; expressions at src/pic1dp_interaction.F90:274-337).
struct SpeciesConst {
  double Z, m;          // charge, mass
  double den, beam;     // density, 1 - density
  double v0, T;
  double tm, tm2;       // T/m, T2/m
  double two_tm, two_tm2;  // 2*T/m, 2*T2/m
  double stm, stm2;     // sqrt(T/m), sqrt(T2/m)
  // reciprocals RN(1/c): exact products when every divisor is a power of two, else div_const
  double r_m, r_T, r_tm, r_tm2, r_two_tm, r_two_tm2, r_stm, r_stm2;
  int pow2;             // 1: all divisors above are powers of two
  int unit;             // 1: m = T = T2 = 1 (T/m = sqrt(T/m) = 1, 2T/m = 2): divisions vanish
  int zunit;            // 1: |Z| = 1 -- with unit, the whole-step kernels' unit instances take dt Z from the host (StepArgsDev::dtz_*)
  int fastc;            // 1: a/c by reciprocal + two FMA corrections for all eight divisors (host-verified)
  // one-exp form of -f0'/f0 (device_math.hpp dlnf0_one_exp; iptcldist 2 and 3): L(v) = (fq2 v + fq1) v + fq0 is
  // the log of the ratio of the two Maxwellians, tmp2 = (fm1 v + fm0) + (fd1 v + fd0) tanh(L / 2)
  int one_exp;          // 1: the marker kernels use it (default; PIC1DP_DLNF0=ref: the reference's operation order)
  double fq2, fq1, fq0, fm1, fm0, fd1, fd0;
};
// one species of the input file (src/pic1dp_input.F90:43-72) -> the constants above (host; species.cpp).
// PIC1DP_UNIT_SPECIALISATION, PIC1DP_FAST_DIVC, PIC1DP_DLNF0 (tuning / cross-check) are read here.
struct SpeciesInput {
  int iptcldist;
  double charge, mass, temperature, temperature2, density, v0;
};
SpeciesConst make_species_const(const SpeciesInput &in, int species_index);

struct GridConst {
  double lx, dnx, dt_full;
  double rlx;    // RN(1/lx), for the exact division by the constant lx
  double rlx_lo; // RN(1/lx - rlx): the low part of the two-operation quotient (const_mul.hpp)
  int nx;
  int mul2;      // 1: the host has PROVEN fma(rlx, x, RN(rlx_lo x)) = RN(x / lx) for every x (const_mul_decide);
                 // 0: locate divides in Markstein's five operations
  int gcopies, gstride;  // copies of the species accumulators in memory (power of two) and doubles between them:
                         // workgroup b flushes into copy b % gcopies (fewer atomics per address), the field
                         // kernels add the copies up
};

// Marker storage.  The four arrays of a species (x, v, w, p) are NOT four separate
// allocations: they are interleaved in tiles of TILE markers,
//     [ x tile | v tile | w tile | p tile ] [ x tile | v tile | ... ] ...
// so that marker i of array k lives at slab[(i / TILE) * 4 * TILE + k * TILE + i % TILE].
// Why: the second sub-step's kernel runs seven streams at once (x, v, w, p read; x, v,
// w written back).  As four independent arrays their relative position in physical
// memory -- which the allocator, not the program, decides -- moved that kernel between
// 1.00 and 1.16 ms at 1e8 markers (DRAM bank/channel interference: tools/placement_probe.py
// maps kernel time against the array-to-array distance), and a pure 4-read / 3-write
// stream reached 5.0 TB/s.  Interleaved at 32 KiB the distances are fixed by the layout:
// the same stream runs at 6.3 TB/s wherever the slab lands (tools/layout_probe.py;
// 8 KiB: 5.3, 128 KiB: 5.3).  PIC1DP_TILE_LOG2=0 builds the untiled variant (arrays a
// 2 MiB multiple apart in one slab) for A/B measurements.
#ifndef PIC1DP_TILE_LOG2
#define PIC1DP_TILE_LOG2 12
#endif
constexpr int TILE_LOG2 = PIC1DP_TILE_LOG2;
constexpr int64_t TILE = static_cast<int64_t>(1) << TILE_LOG2;
static_assert(TILE_LOG2 == 0 || TILE_LOG2 >= 7, "a wave's 64 pairs must not straddle a tile");
// offset of marker i inside an array of a slab (arrays start k * TILE apart)
__host__ __device__ constexpr int64_t tidx(int64_t i) {
  return TILE_LOG2 ? (((i >> TILE_LOG2) << (TILE_LOG2 + 2)) + (i & (TILE - 1))) : i;
}
// the same for marker PAIRS, in double2 units
__host__ __device__ constexpr int64_t tidx2(int64_t j) {
  return TILE_LOG2 ? (((j >> (TILE_LOG2 - 1)) << (TILE_LOG2 + 1)) + (j & (TILE / 2 - 1))) : j;
}
// doubles of a slab holding n markers, and where array k (0 x, 1 v, 2 w, 3 p) starts
inline int64_t slab_array_stride(int64_t n) {
  if (TILE_LOG2) return TILE;
  // untiled A/B build only (-DPIC1DP_TILE_LOG2=0): arrays a 2 MiB multiple apart
  const int64_t unit = (2 << 20) / 8;
  return (n + unit - 1) / unit * unit;
}
inline int64_t slab_doubles(int64_t n) {
  return TILE_LOG2 ? (n + TILE - 1) / TILE * 4 * TILE : 4 * slab_array_stride(n);
}

// Kind 1 of the charge sum (pic1dp_hip_set_charge_sum): every contribution wl q, (1 - wl) q of the
// deposit is rounded once to a whole number n = rint(c 2^-e) of quanta 2^e (e per species, from the input alone:
// pic1dp_hip_charge_quantum) and the integers are summed exactly -- in the LDS as two u64 words per cell (n's low 32
// bits, unsigned, and its high half, signed), globally as two int64 rows per species (hi, lo), across ranks element by
// element.  Integer additions commute: the total does not depend on the order of waves, workgroups, launches or ranks.
// |n| >= 2^62 is not summed: it counts in `ovf` (host-visible), and the next synchronising call reports it.
struct FxArgs {
  long long *acc;            // [2][nx] this species' (hi, lo) rows, or null: kind 0 (FP64 atomics)
  double inv_q;              // 2^-e
  unsigned long long *ovf;   // host-visible counter of contributions beyond 2^62 quanta
};
constexpr double FX_LIMIT = 0x1p62;
// hi 2^32 + lo (lo any u64: normalised first) -> the nearest double, ties to even: ONE rounding of the exact
// integer, what Python's float(int) gives.  Integer operations only, and an exact conversion of a < 2^54 integer
// at the end: nothing here relies on how the compiler lowers a wide integer-to-double conversion.
__host__ __device__ inline double fx_limbs_to_double(long long hi, unsigned long long lo) {
  hi += static_cast<long long>(lo >> 32);
  lo &= 0xffffffffull;
  const bool neg = hi < 0;
  unsigned long long uh, ul;  // |value| = uh 2^32 + ul, ul < 2^32
  if (!neg) {
    uh = static_cast<unsigned long long>(hi);
    ul = lo;
  } else if (lo == 0) {
    uh = 0ull - static_cast<unsigned long long>(hi);
    ul = 0;
  } else {
    uh = 0ull - static_cast<unsigned long long>(hi) - 1ull;
    ul = (1ull << 32) - lo;
  }
  double r;
  if (uh < (1ull << 21)) {  // below 2^53: exact
    r = static_cast<double>(static_cast<long long>((uh << 32) | ul));
  } else {
    const int bits = 96 - __builtin_clzll(uh);  // bit length of the magnitude (54 ... 95)
    const int sh = bits - 53;                   // 1 ... 42
    unsigned long long top, rem, half;
    if (sh <= 32) {
      top = (uh << (32 - sh)) | (ul >> sh);
      rem = ul & ((1ull << sh) - 1ull);
    } else {
      top = uh >> (sh - 32);
      rem = ((uh & ((1ull << (sh - 32)) - 1ull)) << 32) | ul;
    }
    half = 1ull << (sh - 1);
    if (rem > half || (rem == half && (top & 1ull))) top += 1ull;  // (top may reach 2^53: still exact)
    r = ldexp(static_cast<double>(static_cast<long long>(top)), sh);
  }
  return neg ? -r : r;
}

// One particle set = the three pushed arrays of a species (array bases inside a slab).
struct PSet {
  double *x, *v, *w;
};

struct PushArgs {
  PSet src;       // state the derivatives are evaluated at (particle_x/v/w)
  PSet base;      // RK base (particle_*_bak); == src for irk 1
  PSet dst;       // where the pushed state goes
  const double *p;
  const double *E;  // [nx] field_electric
  double *rho;      // [nx] this species' charge accumulator (fused deposit)
  int64_t np;
  double dt;        // 0.5*dt (irk 1) or dt (irk 2)
  GridConst g;
  SpeciesConst s;
  int iptcldist, deltaf, linear, irk;
  FxArgs fx;        // kind 1 of the charge sum: the fused deposit's exact accumulators (acc null: rho)
};

// geometry of the output_ptcldist histograms (src/pic1dp_output.F90:203-205,243-247)
struct DistGeom {
  double lx, vmax;
  int nxo, nvo;   // nx_opd, nv_opd
  // the two divisions of :243, :247 are divisions by run-time constants: rlx = RN(1/lx) (GridConst::rlx), dv = vmax * 2.0
  // and rdv = RN(1/dv); vfast = 1: the host vouches for div_const's five operations on dv (hostcheck.cpp), else the
  // hardware's division.  Bit for bit the IEEE quotients either way (device_math.hpp div_lx).
  double rlx, dv, rdv;
  int vfast;
};
DistGeom make_dist_geom(double lx, double vmax, int nxo, int nvo);
// lx, nx, dnx, rlx and the two-operation quotient's decision (const_mul.hpp) as create() fills them; dt_full and the
// accumulator copies are the caller's (hostcheck.cpp)
GridConst make_grid_const(double lx, int nx);
// scales of the histograms' 64-bit fixed-point sums in a workgroup's LDS copy (device_diag.hpp): plane k (markers, p, w)
// is summed as RN(term * sc[k]); a |p| / |w| beyond bound[k] makes the pass say so instead (the host repeats it in doubles)
struct DistScale {
  double sc[3];     // 2^e per plane
  double inv[3];    // 2^-e
  double bound[3];  // |q_k| the scale allows
};
// the scales for a pass of `blocks` workgroups over np markers whose |p|, |w| stay below bound_p, bound_w (<= 0: unknown);
// false: no fixed-point pass possible (sum in doubles).  (launch_policy.cpp: host arithmetic)
bool make_dist_scale(int64_t np, int blocks, bool deltaf, double bound_p, double bound_w, DistScale *fx, int threads = 1024);
// doubles per workgroup in the partial sums of a diagnostics pass (k_ptcldist, k_step_full<DIAG>): the kinetic sums,
// max |p|, max |w|, the fixed-point pass's overflow flag
constexpr int DIAG_PART = 6;
// launch shape of a diagnostics pass (launch_policy.hpp diag_launch)
struct DiagLaunch {
  int blocks, threads;
  bool lds;       // the histograms as a copy per workgroup in its LDS; false: straight into memory
  size_t bytes;   // dynamic LDS
  bool nt;        // non-temporal marker loads
};

// One pass of pic1dp_hip_moments over a species' markers (launch_policy.hpp moments_plan; kernels_moments.hip k_moments): the
// planes it holds in the workgroup's LDS are powers `kmask` (bit k: v^k) of the weight sets p and / or w, in output order
struct MomentsPass {
  int blocks, threads;
  bool nt;          // non-temporal marker loads
  size_t bytes;     // dynamic LDS: the planes, [plane][cell] doubles, and nothing else
  bool p, w;        // the weight sets of this pass (both: p's planes first)
  int kmask;        // 0xF, 0x3 or 0xC
  int first_plane;  // where the pass's first plane lies in the output [sets selected][4][nx], in planes
  int planes;       // planes of the pass
};
constexpr int MOMENTS_MAX_PASSES = 4;
struct MomentsPlan {
  int selected;     // planes asked for: 4 or 8
  int group;        // planes a pass holds: 8, 4 or 2
  int npass;
  MomentsPass pass[MOMENTS_MAX_PASSES];
};

// One pass of pic1dp_hip_power over a species' markers (launch_policy.hpp power_plan; kernels_power.hip k_power): the planes
// of `sets` weight sets from `first_set` on (of the sets selected, in output order), in the workgroup's LDS behind the E
// tile (lds) or straight in memory
struct PowerPass {
  int blocks, threads;
  bool nt;          // non-temporal marker loads
  size_t bytes;     // dynamic LDS: the E tile, and behind it the pass's planes where lds
  bool p, w;        // the weight sets of this pass (both: p's plane first)
  bool lds;         // the planes as a copy per workgroup in its LDS; false: straight into memory
  int first_set;    // where the pass's first plane lies in the output, in weight sets
  int sets;         // weight sets of the pass
};
constexpr int POWER_MAX_PASSES = 2;
struct PowerPlan {
  int selected;     // weight sets asked for: 1 or 2
  int npass;
  size_t tile;      // bytes of the E tile: nx + 1 doubles, rounded up to 16
  size_t plane;     // bytes of one plane: nx_opd * nv_opd doubles
  PowerPass pass[POWER_MAX_PASSES];
};

// launch shape of the state digest's pass (launch_policy.hpp digest_launch)
struct DigestLaunch {
  int blocks, threads;
  bool nt;        // non-temporal marker loads
};

// dynamic LDS any kernel may ask for: 160 KiB per CU minus 1 KiB, the most static LDS a kernel that asks for more than
// 64 KiB holds (the particle kernels' exp table; k_field_fd: 144 B)
constexpr size_t PARTICLE_LDS_CAP = 159 * 1024;

struct LaunchCfg {
  int threads;   // per workgroup
  int blocks;    // grid size
  size_t lds;    // dynamic LDS bytes
};

// Every kernel launch of the library.  Above 64 KiB of dynamic LDS the kernel opts in to PARTICLE_LDS_CAP, on every call
// (idempotent and cheap, and for whichever device is current); beyond the cap nothing is launched.
template <typename K, typename... Args>
hipError_t launch_kernel(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &...args) {
  if (lds > 64 * 1024) {
    if (lds > PARTICLE_LDS_CAP) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       PARTICLE_LDS_CAP);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
  return hipGetLastError();
}

// run-time bools as compile-time arguments: f(std::bool_constant...), one per bool
template <class F>
hipError_t with_bools(F &&f) {
  return f();
}
template <class F, class... Bools>
hipError_t with_bools(F &&f, bool first, Bools... rest) {
  auto next = [&](auto B) { return with_bools([&](auto... r) { return f(B, r...); }, rest...); };
  return first ? next(std::true_type{}) : next(std::false_type{});
}

struct FieldArgs {
  double *rho_sp;        // [rho_copies][nspecies][nx] raw per-species deposits (zeroed after use)
  int rho_copies, rho_stride;  // copies the particle kernels flush into, doubles between them (GridConst::gcopies)
  double *charge;        // [nx] charge2 / charge1 (local sum, all-reduced in place)
  double *chargeden;     // [nx]
  double *E;             // [nx]
  double *mode_re, *mode_im;   // [nmode]
  const double *fre, *fim;     // [nmode][nx] cos / -sin tables
  const double *grad_inv;      // [nmode]
  double *history;       // energy slot to write, or nullptr
  int nx, nmode, nspecies, deltaf;
  int npe;               // reference ranks reproduced: > 1 takes the forward sums in the npe-rank order (MPI-AIJ row
                         // blocks, device_field.hpp rank_block) and the inverse's per row with the row's own rank's mode
                         // entries first (inverse_row); 1: the one-rank ascending order
  int tab_lds;           // 1: stage the tables in LDS (they fit)
  int chain_mfma;        // 1: the serial forward sums of the one-rank order (up to eight kept modes) through the FP64
                         // matrix unit (device_field.hpp chain_rows_mfma) -- set by create() only if the device gives the
                         // sequential sums bit for bit that way (launch_chain_selftest); 0: a chain of additions in one lane
  double lx, dnx, sc_re, sc_im;
  double Z[8], n0[8];
};

// what the host knows of the one kept mode's tables (pred_kind 2): their sums (full-f offset) and their Gram
// matrix (kept-mode reconstruction of chargeden for the call-site path)
struct PredTab {
  double sum_fre, sum_fim, g11, g22, g12;
};

// one-hop charge exchange between the GPUs of a node (kernels_field.hip exchange_charge)
constexpr int XCHG_MAX_RANKS = 16;
struct XchgArgs {
  double *slots[XCHG_MAX_RANKS];               // every rank's slot area [2][nranks][nx] as mapped here
  unsigned long long *flags[XCHG_MAX_RANKS];   // every rank's flag area [2][XCHG_MAX_RANKS]
  unsigned long long *err;                     // host-visible error word (0 = fine)
  unsigned long long epoch;                    // number of this exchange, from 1
  long long timeout_ticks;                     // wall_clock64 ticks (100 MHz) a rank waits for its peers
  int rank, nranks;
  int local_in_charge;                         // 1: this rank's charge2 is already in FieldArgs::charge
  int vstride;                                 // doubles per (parity, rank) slot: XCHG_MAX_VEC * nx
  unsigned long long *ticks;                   // null, or [2] device words: wall-clock ticks (100 MHz) spent inside
                                               // exchanges so far (stores, the wait for the peers, the sum) and their number
};
// The TAIL of a one-pass marker launch on several ranks (device_xchg.hpp step_tail; k_step_one<PRIV>, k_step_sums, the
// last species launched): the last workgroup to finish forms this rank's packed vector [charge2 | six sums | pad] from the
// accumulators (re-zeroed) -- what k_charge_pack_sums did in a launch of its own -- and either leaves it in `pack` for
// the all-reduce that follows on the stream (mode 1) or stores it into every rank's exchange slots (mode 2), so that
// the field launch only waits for the flags, adds in rank order and solves.
struct StepTail {
  int mode;                    // 0 none, 1 pack for one all-reduce, 2 post into the peers' exchange slots
  unsigned int *ticket;        // device word, zero between launches: workgroups that have finished
  double *rho_sp;              // [rho_copies strides][nspecies][nx] the accumulators of ALL species (read, re-zeroed)
  int rho_copies, rho_stride, nspecies, nx;
  double Z[8];
  double *sums;                // [PRED_SUM_COPIES][8] the six sums' copies (read, re-zeroed)
  double *pack;                // mode 1: [nx + 8]
  XchgArgs x;                  // mode 2
};

// A whole-step launch whose PROLOGUE solves the field of the previous step itself (kernels_step.hip FUSED; one rank, one
// kept mode, prediction as six sums): every workgroup forms charge2 / chargeden from the accumulators the previous
// launch deposited into, runs the forward sums in the reference's order (the same device functions as the field
// kernels: device_field.hpp), and writes E0 and Eh of this step straight into its LDS tiles -- one launch per time
// step instead of two; workgroup 0 also writes what the field kernel would have left in memory.  The accumulators
// rotate through three buffers: read (deposited by the previous launch), deposit (this launch), zeroed by workgroup 0
// (read by the previous launch: nobody touches it any more).
struct FusedSolve {
  int on;                 // 0: the launch stages E0 / Eh from memory
  FieldArgs f;            // rho_sp: the accumulators to READ (left as they are); charge, chargeden, E, mode_re / mode_im,
                          // history: outputs of workgroup 0
  PredTab pt;
  const double *pred_in;  // [PRED_SUM_COPIES][8] the previous launch's six sums (read, left as they are)
  double *E_h, *mode_h;   // workgroup 0: this step's half-step field and its kept mode (re, im)
  double *zero_rho;       // workgroup 0 zeroes zero_rho[0 .. zero_rho_n) and zero_pred[0 .. 8 PRED_SUM_COPIES)
  int64_t zero_rho_n;
  double *zero_pred;
};

// whole-time-step path, state updated in place, half-step state recomputed: what the marker kernels
// (kernels_step.hip) receive
struct StepArgsDev {
  double *x, *v, *w;   // particle_x/v/w, updated in place by the full kernel
  const double *p;
  const double *E0;    // field at the start of the step
  const double *Eh;    // field after the first sub-step (full kernel only)
  double *rho;         // this species' charge accumulator
  int64_t np;
  double dt_half, dt_full;
  double dtz_half, dtz_full;   // dt_half Z, dt_full Z (launch_step): the unit instances' step constants with the charge folded in
  GridConst g;
  SpeciesConst s;
  int nt;              // 1: non-temporal loads/stores (state larger than the Infinity Cache)
  int plain_chunks;    // one-pass kernels, nt = 1: the first plain_chunks 64-pair chunks of the slab use plain accesses all
                       // the same -- the share of the state kept in the cache (launch_policy.hpp stream_plain_chunks)
  double *t2;          // [np + 2] -f0'/f0 at the step-start velocity, carried from k_step_half to k_step_full (or null)
  // full kernel only: the diagnostics of output_all taken on the new state in the same pass (kernels_step.hip DIAG)
  DistGeom dg;
  double *dist_out;      // histograms [3*nxo*nvo + 3*nvo] of this species (accumulated with atomics), or null
  double *dist_partial;  // [gridDim][3] kinetic sums per workgroup
  // full kernel only: also predict the charge of the NEXT step's first sub-step (StepFamily); pred null = no.
  // tabA/tabB: [pred_nm][nx] mode tables with E = sum_m re_m*A_m + im_m*B_m.  pred: Tiles, [1 + 2*pred_nm][nx]
  // accumulators of this species (R0, RA_m, RB_m); the six sums, [PRED_SUM_COPIES][8] -- K0c K1c K2c K0s K1s K2s shared
  // by all species (Z folded in), in copies.  t2_mode: 0 no carry of -f0'/f0 through t2, 1 write it for the next step,
  // 2 read this step's and write the next step's
  const double *tabA, *tabB;
  double *pred;
  int pred_nm, t2_mode;         // pred_nm: the kept modes
  const double *eh_re, *eh_im;  // k_step_sums: Eh is not staged but formed from the tables and its kept mode (Eh = re A +
                                // im B, bit for bit what the solve wrote)
  double snx, pred_k;           // the prediction: nx / lx, and dt/2 Z/m (launch_step)
  FusedSolve fused;             // the six sums only: the prologue solves the previous step's field (E0, Eh, eh_re / eh_im unused)
  StepTail tail;                // the six sums only, several ranks: the last workgroup packs / posts this rank's charge (mode 0: no)
  DistScale dscale;             // k_step_full<DIAG>: the histograms as fixed-point sums (diag_fx != 0)
  int diag_fx;
  int dyn_tail;                 // every whole-step kernel: sixteenths of a workgroup's chunks that its waves draw from an LDS
                                // counter (0: all dealt)
  double *fxb;                  // Tiles: [2] device bounds on |q|, |c| of this species, for the tiles' fixed-point sums
  double fx_markers, fx_cap;    // ... the most markers one workgroup of this launch takes, and 2^61 over it (launch_step)
  FxArgs fx;                    // kind 1 of the charge sum (k_step_half / k_step_full<EXACT>): the exact accumulators (acc null: rho)
#ifdef PIC1DP_TUNING       // tuning build, PIC1DP_PLAIN_ROWS=1 (k_step_one): > 0: every plain_every-th grid-stride row is plain instead
  int plain_every;          // of the first plain_chunks chunks -- the same share of the state, spread over the launch
#endif
#ifdef PIC1DP_TUNE_STAMPS  // tuning build (tools/stamp_probe.sh): [gridDim][8] wall-clock stamps of the phases of a workgroup
  unsigned long long *stamps;
#endif
};
// the kernel family of a full step that predicts (pred non-null); every other launch takes k_step_half / k_step_full
enum class StepFamily {
  Tiles,        // k_step_one<NM>: prediction tiles of pred_nm kept modes
  Sums,         // k_step_sums: one kept mode as six global sums, for grids whose tiles outgrow the LDS
  PrivateSums,  // k_step_one<PRIV>: the six sums in thread-private LDS slots (E0, Eh and the table tiles fit the LDS)
};
// a whole-step launch: the kernel arguments and what picks the instantiation on the host
struct StepArgs {
  StepArgsDev d;
  int iptcldist, deltaf, linear;
  StepFamily family;
};
#ifndef PIC1DP_PRED_MAX_MODES
#define PIC1DP_PRED_MAX_MODES 3
#endif
constexpr int PRED_MAX_MODES = PIC1DP_PRED_MAX_MODES;  // kept modes k_step_one's prediction tiles are instantiated for: 1 ... 3.  (Round 4
                                    // built three and four with double sums and lost to the two passes; with the fixed-point
                                    // sums of round 6 three win -- 1.20 against 1.40 ms at 1e8 markers --, four were not rebuilt)
// pred_kind 2: the six sums (padded to 8) are kept in this many copies -- workgroup b of the marker kernel adds into
// copy b % PRED_SUM_COPIES, the field kernels add the copies up: six addresses shared by all workgroups serialise
constexpr int PRED_SUM_COPIES = 16;
// dynamic LDS of the whole-step kernels k_step_half / k_step_full: E0 tile, Eh tile (full only), rho tile (exact: kind 1 of
// the charge sum, two words per cell)
inline size_t step_lds_bytes(int nx, bool full, bool exact = false) {
  const size_t ne = static_cast<size_t>((nx + 2) & ~1);
  return sizeof(double) * ((full ? 2 : 1) * ne + (exact ? 2 : 1) * ((static_cast<size_t>(nx) + 2) & ~static_cast<size_t>(1)) +
                           2);  // (+ the drawn chunks' counter, 16-byte slot)
}
// dynamic LDS of k_step_sums: E0, A, B tiles (with guard cell), rho copies, reduction scratch
inline size_t step_sums_lds_bytes(int nx) {
  const size_t ne = static_cast<size_t>((nx + 2) & ~1);
  return sizeof(double) * (3 * ne + ((static_cast<size_t>(nx) + 2) & ~static_cast<size_t>(1)) + 96);  // [6][16] scratch
}
// dynamic LDS of k_step_one: E0, Eh tiles (with guard cell), the tables cell by cell (nx + 1 cells of 2 nm), rho
// copies, the prediction accumulators cell by cell (nx + 2 cells of 1 + 2 nm)
inline size_t step_one_lds_bytes(int nx, int nm) {
  const size_t ne = static_cast<size_t>((nx + 2) & ~1);
  return sizeof(double) * (2 * ne + (static_cast<size_t>(nx) + 1) * 2 * nm +
                           ((static_cast<size_t>(nx) + 2) & ~static_cast<size_t>(1)) +
                           (static_cast<size_t>(nx) + 2) * (1 + 2 * nm) + 2);  // (+ the drawn chunks' counter)
}
// dynamic LDS of k_step_one<PRIV>: E0, Eh tiles, the one mode's tables cell by cell (nx + 1 cells of 2), rho copies,
// six private sums per thread, reduction scratch
#ifndef PIC1DP_PRIV_THREADS
#define PIC1DP_PRIV_THREADS 768  // (tuning builds: 1024 = one workgroup of sixteen waves per CU, tools/ab_variant_libs.sh)
#endif
constexpr int STEP_PRIVATE_THREADS = PIC1DP_PRIV_THREADS;  // k_step_one<PRIV> is launched with exactly this many threads per workgroup
inline size_t step_one_private_lds_bytes(int nx, int threads = STEP_PRIVATE_THREADS) {
  const size_t ne = static_cast<size_t>((nx + 2) & ~1);
  return sizeof(double) * (2 * ne + (static_cast<size_t>(nx) + 1) * 2 +
                           ((static_cast<size_t>(nx) + 2) & ~static_cast<size_t>(1)) +
                           6 * static_cast<size_t>(threads) + 16);
}
// dynamic LDS of the DIAG variant beyond the grid tiles: histograms + reduction scratch
inline size_t step_diag_lds_bytes(int nx, int nxo, int nvo) {
  (void)nx;  // the rho region of step_lds_bytes ends 16-byte aligned
  return sizeof(double) * (3 * static_cast<size_t>(nxo) * nvo + 3 * static_cast<size_t>(nvo) + 16);
}
// full = false: first sub-step (deposit of the half-step state, nothing stored)
// full = true : second sub-step (recompute half-step state, push, deposit, store)
// (a.d's snx, pred_k, fx_markers and fx_cap are derived here)
hipError_t launch_step(StepArgs a, bool full, const LaunchCfg &lc, hipStream_t st);

// push (+gather) with or without the fused wrap+deposit
hipError_t launch_push(const PushArgs &a, bool fused_deposit, const LaunchCfg &lc, hipStream_t st);
// wrap + deposit of q (= w or p) at x, x stored back: into rho, or -- fx.acc non-null -- into the exact accumulators
// of kind 1 (lc.lds: 16 B per cell and the guard cell)
hipError_t launch_deposit(double *x, const double *q, double *rho, const FxArgs &fx, int64_t np, const GridConst &g,
                          const LaunchCfg &lc, hipStream_t st);


// vectors of nx doubles one exchange can carry: charge2 + the 1 + 2 * PRED_MAX_MODES prediction slices
constexpr int XCHG_MAX_VEC = 2 + 2 * PRED_MAX_MODES;
// both fields of a one-pass step in one launch: the new state's field from its deposited charge, then the
// NEXT step's half-step field from k_step_one's prediction (x1: the ONE exchange of a multi-rank step -- charge2
// and the Z-weighted prediction slices travel together --, or null)
struct PairArgs {
  double *pred;     // kind 1: [nspecies][1 + 2 nmode][nx]; kind 2: [PRED_SUM_COPIES][8] the six sums; consumed (re-zeroed)
  double *E_h;      // [nx] half-step field of the next step
  double *mode_h;   // [2 nmode] its kept modes (re..., im...)
  double *cd_h;     // [nx] its charge density (kind 1: scratch; kind 2: the kept mode's content of it, for the call sites' adoption)
  double *pack;     // null, or what k_charge_pack made, already summed over ranks
  int kind;         // 1 tiles, 2 sums
  PredTab pt;       // kind 2
  int posted;       // kind 2 with x1: the marker launch's tail has stored this rank's vector and flag already (StepTail mode 2)
};
// doubles k_charge_pack writes / one exchange of a one-pass step carries per rank:
// kind 1: charge2 + the 1 + 2 nmode Z-weighted prediction slices; kind 2: charge2 + the six sums (padded to 8)
constexpr size_t pack_doubles(int nx, int nmode, int kind) {  // (constexpr: host and device, field_lds.hpp)
  return kind == 2 ? static_cast<size_t>(nx) + 8 : static_cast<size_t>(2 + 2 * nmode) * nx;
}
// this rank's charge2 and prediction packed for one all-reduce (accumulators re-zeroed)
hipError_t launch_charge_pack(const FieldArgs &f, double *pred, int nm_pred, int kind, double *pack, hipStream_t st);
hipError_t launch_field_solve_pair(const FieldArgs &f, const PairArgs &pa, const XchgArgs *x1, hipStream_t st);
// kind 2, call-site path: the six sums K (summed over ranks) + the field's kept mode -> field_chargeden with the
// kept-mode content of the next first sub-step's charge density; pred (or null) is re-zeroed
hipError_t launch_pred_chargeden(const FieldArgs &f, const PredTab &pt, double *pred, const double *K, hipStream_t st);
// kind 2, call-site path, one rank: launch_pred_chargeden (from this rank's copies of the sums) and the mode-filter
// solve in one launch
hipError_t launch_field_solve_pred_sums(const FieldArgs &f, const PredTab &pt, double *pred, hipStream_t st);
// kind 2, call-site path, several ranks: this rank's six sums into the head of f.charge (rest zero), pred re-zeroed
hipError_t launch_pred_to_charge(const FieldArgs &f, double *pred, hipStream_t st);
// k_step_one's prediction accumulators [nspecies][1 + 2 nm][nx] + the field's kept modes -> this rank's
// charge2 of the next first sub-step in f.charge; the accumulators are re-zeroed
hipError_t launch_pred_combine(const FieldArgs &f, double *pred, int nm_pred, hipStream_t st);
// launch_pred_combine, the scaling into f.chargeden and the mode-filter solve in one launch (call sites, one rank)
hipError_t launch_field_solve_pred(const FieldArgs &f, double *pred, int nm_pred, hipStream_t st);
// local charge + exchange: the summed charge1 into f.charge
hipError_t launch_charge_exchange(const FieldArgs &f, const XchgArgs &x, hipStream_t st);
// local charge + exchange + chargeden + field solve in one launch
hipError_t launch_field_solve_xchg(const FieldArgs &f, const XchgArgs &x, hipStream_t st);

// kind 1 of the charge sum.  acc: [nspecies][2][nx] int64 (hi row, lo row per species).
// normalise: lo <- lo mod 2^32, hi <- hi + (lo >> 32) (the packet a sum over ranks adds element by element)
hipError_t launch_fx_normalise(long long *acc, int nspecies, int nx, hipStream_t st);
// rho_sp[s][i] (copy 0) <- the double nearest to (hi 2^32 + lo) times q[s] = 2^e_s; acc re-zeroed
hipError_t launch_fx_to_rho(long long *acc, double *rho_sp, int nspecies, int nx, const double *q, hipStream_t st);
// the normalised packet summed over the ranks of the one-hop exchange (slots of at least 2 nspecies nx), in place
hipError_t launch_fx_exchange(long long *acc, int nspecies, int nx, const XchgArgs &x, hipStream_t st);
// charge2 = sum_s rho_sp[s]*Z_s ; rho_sp = 0      (src/pic1dp_interaction.F90:81-128)
hipError_t launch_charge_local(const FieldArgs &f, hipStream_t st);
// chargeden from charge (:138-148) only; with_local folds launch_charge_local in
hipError_t launch_chargeden(const FieldArgs &f, bool with_local, hipStream_t st);
// chargeden from charge (:138-148) then field_solve_electric; with_local runs
// launch_charge_local's work first in the same kernel (single-rank path)
hipError_t launch_field_solve(const FieldArgs &f, bool with_local, bool from_chargeden,
                              hipStream_t st);
// Transform 1 of the mode-filter solve (pic1dp_hip_set_field_transform; kernels_fft.hip): the DFT of
// chargeden by a one-workgroup mixed-radix FFT in LDS instead of the dense tables.  Supported: nx = 2^a 3^b 5^c,
// 2 <= nx <= FFT_MAX_NX, odd nx up to FFT_MAX_ODD_NX (two complex buffers of nx points in LDS).
constexpr int FFT_MAX_NX = 8192, FFT_MAX_ODD_NX = 3375, FFT_MAX_PASSES = 16;
struct FftArgs {
  const double2 *tw;       // [nx] w_nx^k = e^{-2 pi i k / nx}, the angle reduced exactly on the host
  const int *bin_start;    // [nx + 1] the kept modes of bin b (= m mod nx) are bin_mode[bin_start[b] .. bin_start[b + 1])
  const int *bin_mode;     // [nmode] mode indices by bin, ascending within a bin
  const int *mode_bin;     // [nmode] the bin of each kept mode
  int n;                   // complex points transformed: nx / 2 (nx even: real packing) or nx
  int npass;
  int radix[FFT_MAX_PASSES];
};
bool fft_supported(int nx);
// the plan of nx for the kept modes `modes`: radices into p, twiddles and the bins into device buffers (allocated when
// null, synchronous copies)
hipError_t fft_plan_upload(int nx, const int32_t *modes, int nmode, FftArgs &p, double **d_tw, int **d_idx);
// launch_field_solve with the FFT: chargeden (unless from_chargeden), then one launch -- forward FFT, the kept modes, the
// Hermitian spectrum of E, inverse FFT, E (+ field energy)
hipError_t launch_field_fft(const FieldArgs &f, const FftArgs &p, bool with_local, bool from_chargeden, hipStream_t st);
// opt-in alternative solve (all modes): finite-difference Poisson equation as a
// tridiagonal system, parallel cyclic reduction in LDS; chargeden -> E (+ energy)
hipError_t launch_field_fd(const double *chargeden, double *E, double *history, int nx, double lx,
                           double dnx, hipStream_t st);
// The serial sums of nrows (<= 16) rows of n generated doubles two ways: out[0 .. nrows) chain_sum_lds, out[16 .. 16 + nrows)
// chain_rows_mfma -- create() compares them with the host's sequential sums
hipError_t launch_chain_selftest(const double *v, int nrows, int n, double *out, hipStream_t st);
// int E^2 dx into *out (device)
// output_all's record gathered on the device: up to PACK_MAX_SEGMENTS ranges copied into one contiguous buffer, which then
// crosses PCIe in ONE transfer (a small device-to-host copy costs the stream ~10 us whatever its size; a record had 5 + 2 per species)
constexpr int PACK_MAX_SEGMENTS = 5 + 2 * 8;
struct PackArgs {
  const double *src[PACK_MAX_SEGMENTS];
  unsigned dst[PACK_MAX_SEGMENTS];  // offset in the record, in doubles
  unsigned n[PACK_MAX_SEGMENTS];
  int count;
};
hipError_t launch_pack_record(const PackArgs &a, double *out, hipStream_t st);
hipError_t launch_field_energy(const double *E, int nx, double lx, double dnx, double *out,
                               hipStream_t st);

// per-block partial sums of v^2, v^2 p, v^2 w over markers [i0, i0 + n) -> partial[blocks][3]
hipError_t launch_energy_sums(const double *v, const double *p, const double *w, int64_t i0, int64_t n,
                              double *partial, int blocks, hipStream_t st);
// contiguous buffer <-> markers [i0, i0 + n) of one array of a slab
hipError_t launch_tile_scatter(double *arr, int64_t i0, const double *src, int64_t n, hipStream_t st);
hipError_t launch_tile_gather(const double *arr, int64_t i0, double *dst, int64_t n, hipStream_t st);
// markers [0, n) of one array copied between two slabs of the same geometry
hipError_t launch_tile_copy(double *dst, const double *src, int64_t n, hipStream_t st);
// raw (x,v) and v histograms of output_ptcldist into out =
// [markr_xv | total_xv | pertb_xv | markr_v | total_v | pertb_v] (accumulated)
// In the same pass: partial[dl.blocks][DIAG_PART] = per-workgroup sums of v^2, v^2 p, v^2 w over all np markers, max |p|,
// max |w|, and whether a marker exceeded the bounds of a fixed-point pass; dl = diag_launch(0, ...).
// bound_p, bound_w > 0: the (x, v) histograms as 64-bit fixed-point sums in the LDS (device_diag.hpp DistScale)
hipError_t launch_ptcldist(const double *x, const double *v, const double *p, const double *w, int64_t np, const DistGeom &dg,
                           bool deltaf, double bound_p, double bound_w, double *out, double *partial, const DiagLaunch &dl,
                           int dyn_tail, hipStream_t st, bool *fixed_point);

// Kind 1 of the diagnostics sum (pic1dp_hip_set_diag_sum): every term of the pass -- the corner weights
// times 1, p, w of the (x, v) histograms, and v^2, v^2 p, v^2 w of the kinetic sums -- is rounded once to a whole number
// n = rint(t 2^-e) of quanta 2^e (six per species, from the input alone: pic1dp_hip_diag_quanta) and the integers are
// summed exactly.  acc: [3 planes][2][nx_opd nv_opd] (hi row, lo row, as FxArgs) | [3 sums][2] (hi, lo) |
// [6] terms that were not summed (plane 0..2: 2^44 quanta or more, sum 0..2: 2^62 or more) | [2] padding.
struct DiagFxArgs {
  long long *acc;
  double inv_q[6];   // 2^-e: markr, total, pertb, sum v^2, sum v^2 p, sum v^2 w
};
constexpr double DIAG_FX_LIMIT = 0x1p44;   // a histogram term of this many quanta or more is not summed
constexpr int DIAG_FX_WINDOW_TRIPS = 32;   // a workgroup flushes its LDS copy after this many trips of 2 x 1024 markers
inline size_t diag_fx_limbs(int nxo, int nvo) { return 6 * static_cast<size_t>(nxo) * nvo + 6; }
inline size_t diag_fx_words(int nxo, int nvo) { return diag_fx_limbs(nxo, nvo) + 8; }
// n = rint(t 2^-e) of a term, one rounding to nearest even (t 2^-e itself is exact); false: |n| >= limit or NaN
__host__ __device__ inline bool diag_fx_quantise(double term, double inv_q, double limit, long long *n) {
  const double t = __builtin_rint(term * inv_q);
  if (!(__builtin_fabs(t) < limit)) return false;
  *n = static_cast<long long>(t);
  return true;
}
// the exact pass over markers [0, np) of a species: histograms and kinetic sums into a.acc (accumulated);
// dl = diag_launch(1, ...)
hipError_t launch_ptcldist_exact(const double *x, const double *v, const double *p, const double *w, int64_t np,
                                 const DistGeom &dg, bool deltaf, const DiagFxArgs &a, const DiagLaunch &dl, int dyn_tail,
                                 hipStream_t st);
// ... and the kinetic sums of the tail slots [i0, i0 + n) into the same accumulators
hipError_t launch_energy_sums_exact(const double *v, const double *p, const double *w, int64_t i0, int64_t n,
                                    const DiagFxArgs &a, int nxv, hipStream_t st);
// One pass of the velocity moments on the field grid (kernels_moments.hip; the definition: include/pic1dp_hip.h
// pic1dp_hip_moments) over markers [0, np): out = the species' planes [sets selected][4][nx], zeroed by the caller before a
// call's passes; the pass adds its planes (ps.first_plane ...) with one global atomic per non-zero LDS word and workgroup
hipError_t launch_moments(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst &g,
                          double *out, const MomentsPass &ps, int dyn_tail, hipStream_t st);
// The exact kind of the moments (kernels_moments.hip k_moments_exact; the definition: include/pic1dp_hip.h
// pic1dp_hip_moments_exact): a pass adds whole quanta into acc = the call's limbs [sets selected][4][2][nx] (hi row, lo row,
// as FxArgs) and counts the terms it does not sum (DIAG_FX_LIMIT quanta or more, NaN) in rej = [sets selected][4].  Both are
// zeroed by the caller before a call's passes; launch_moments_exact moves them to the pass's first weight set.
struct MomentsFxArgs {
  long long *acc, *rej;
  double inv_q[4];   // 2^-e[k], by power of v
};
// ps: a pass of moments_plan_exact (its bytes are the planes as 64-bit words)
hipError_t launch_moments_exact(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst &g,
                                const MomentsFxArgs &a, const MomentsPass &ps, int dyn_tail, hipStream_t st);
// One pass of the wave-particle power on the output grid (kernels_power.hip k_power; the definition: include/pic1dp_hip.h
// pic1dp_hip_power) over markers [0, np): E = field_electric [nx]; planes = [sets selected][nx_opd nv_opd] and rest = [sets
// selected], both zeroed by the caller before a call's passes; the pass adds into those of its weight sets (ps.first_set ...)
hipError_t launch_power(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst &g,
                        const DistGeom &dg, const double *E, double *planes, double *rest, const PowerPass &ps, int dyn_tail,
                        hipStream_t st);
// The exact kind of the power (kernels_power.hip k_power_exact; the definition: include/pic1dp_hip.h pic1dp_hip_power_exact;
// DESIGN.md 2.19).  The quantum 2^e follows the field: e = max(e_base + kE, POWER_FX_MIN_E), kE = ceil(log2 max |E|) (0 for
// a field of zeros), which every workgroup takes from the E tile it stages -- a maximum, so the same bits everywhere.
// |x| of a double as its bit pattern orders as an unsigned integer, and a pattern of POWER_FX_NONFINITE or more is an
// infinity or a NaN: one integer maximum is the scale and the flag.
constexpr int POWER_FX_MIN_E = -1000;   // 2^e and 2^-e stay normal doubles for a subnormal field
constexpr unsigned long long POWER_FX_NONFINITE = 0x7ff0000000000000ull;
// ceil(log2 b) of a positive finite double from its bits (sign cleared): fx_limbs.hpp ceil_log2 at every such double
// (tests/power_fx_check.cpp holds the two together)
__host__ __device__ inline int fx_ceil_log2_bits(unsigned long long bits) {
  const int ex = static_cast<int>(bits >> 52);
  const unsigned long long m = bits & 0xfffffffffffffull;
  if (ex != 0) return ex - 1023 + (m != 0ull ? 1 : 0);
  const int top = 63 - __builtin_clzll(m);           // subnormal: b = m 2^-1074, m != 0
  return top - 1074 + ((m & (m - 1ull)) != 0ull ? 1 : 0);
}
// e of a call from e_base = kb + kvm - 40 and the bits of max |E| (finite)
__host__ __device__ inline int power_fx_exponent(int e_base, unsigned long long max_bits) {
  const int e = e_base + (max_bits != 0ull ? fx_ceil_log2_bits(max_bits) : 0);
  return e > POWER_FX_MIN_E ? e : POWER_FX_MIN_E;
}
// acc: the call's limbs, per selected weight set [hi plane nx_opd nv_opd | lo plane | rest hi | rest lo]; rej: [sets
// selected][2] terms not summed (bins, rest); scale: [3] e, the non-finite flag, the bits of max |E| -- written by workgroup 0
// of every pass (the same values).  All zeroed by the caller before a call's passes; launch_power_exact moves acc and rej to
// the pass's first weight set.  A non-finite field: the pass sweeps no marker.
struct PowerFxArgs {
  long long *acc, *rej, *scale;
  int e_base;
};
inline size_t power_fx_set_words(int nxo, int nvo) { return 2 * static_cast<size_t>(nxo) * nvo + 2; }
// ps: a pass of power_plan_exact (its bytes are the tile and the planes as 64-bit words)
hipError_t launch_power_exact(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst &g,
                              const DistGeom &dg, const double *E, const PowerFxArgs &a, const PowerPass &ps, int dyn_tail,
                              hipStream_t st);
// The state digest of one species (kernels_digest.hip; the definition: include/pic1dp_hip.h pic1dp_hip_state_digest).
// Array k (0 x, 1 v, 2 w, 3 p): slot i < np is read from cur[k] (the current particle set), slot i >= np from first[k]
// (set 0, where the tail slots live); out[k] += sum of the mixed words of slots [0, nalloc) (64-bit integer atomics).
struct DigestArgs {
  const double *cur[4], *first[4];
  int64_t np, nalloc;
  unsigned long long *out;   // [4] device words
};
hipError_t launch_state_digest(const DigestArgs &a, const DigestLaunch &dl, hipStream_t st);
// The on-device particle load of one species (kernels_load.hip k_load; the definition: load_seq.hpp): one
// streaming pass over slots [0, nalloc) of set 0's arrays.  Slot i < np is global marker g0 + i; slots beyond hold +0.0.
// maxpw[0], maxpw[1] <- max with the bit patterns of max |p|, max |w| over the valid markers (non-negative doubles order as
// unsigned integers); zeroed by the caller.
struct LoadArgs {
  double *x, *v, *w, *p;
  int64_t np, nalloc;
  unsigned long long g0, key;   // key: load_key(seed offset, species) (kind 1)
  unsigned long long *maxpw;    // [2] device words
  LoadConst k;
};
// launch shape of the load's pass (launch_policy.hpp load_launch)
struct LoadLaunch {
  int blocks, threads;
  bool nt;        // non-temporal stores
};
// markers a workgroup of k_load takes at a time: one tile group, so that the four arrays' tiles are written together
constexpr int64_t LOAD_CHUNK = TILE_LOG2 ? TILE : 4096;
hipError_t launch_load(const LoadArgs &a, int kind, int iptcldist, bool nonlinear, const LoadLaunch &ll, hipStream_t st);

// ---- select and gather markers (kernels_select.hip; the definition: include/pic1dp_hip.h pic1dp_hip_select) ----
// The valid markers are cut into fixed contiguous chunks of SELECT_CHUNK_PAIRS logical pairs (2 j, 2 j + 1): chunk c holds
// pairs [c CP, min((c + 1) CP, np / 2)), and the odd last marker (np odd) belongs to the last chunk.  The cut depends on np
// alone, never on the launch shape: that, and ranks inside a chunk from ballots in lane order, fix the output order.
// 8192 pairs = 128 trips of a one-wave workgroup (eight of 1024 threads) = 256 KiB of x and v: 6104 chunks at 1e8 markers, a
// prefix sum one workgroup does in six rounds, about a chunk per workgroup of the default grid.
constexpr int64_t SELECT_CHUNK_PAIRS = 8192;
// the rule as the kernels take it (pic1dp_select and lx; straddle: x_lo > x_hi)
struct SelectRule {
  double lx, x_lo, x_hi, v_lo, v_hi;
  unsigned long long thin, key, origin;
  int straddle;
};
// launch shape of the count and write passes (launch_policy.hpp select_plan)
struct SelectPlan {
  int64_t chunk_pairs, nchunk;   // nchunk = 0: no valid marker, nothing is launched
  int blocks, threads;           // workgroups take chunks grid-stride; threads a multiple of 64, <= 1024
  bool nt;                       // non-temporal loads of x and v
  int scan_threads;              // the prefix sum's one workgroup
};
// where a species' markers live: x, v, p, w of slots below np (the current set; p has one copy) and of the tail slots (set 0)
struct SelectArrays {
  const double *x, *v, *p, *w;
};
// what a selection hands out, device arrays of `cap` elements each, any of them null
struct SelectOut {
  long long *index;
  double *x, *v, *p, *w;
};
// counts[c] <- markers of chunk c the rule selects, c < nchunk (counts: nchunk + 1 words)
hipError_t launch_select_count(const SelectArrays &a, int64_t np, const SelectRule &r, unsigned long long *counts,
                               const SelectPlan &pl, hipStream_t st);
// counts[c] <- sum of counts[0 .. c - 1] in place, counts[nchunk] <- the total; one workgroup
hipError_t launch_select_scan(unsigned long long *counts, const SelectPlan &pl, hipStream_t st);
// the selected markers of global rank r < cap to out[r], in ascending logical index; prefix: what launch_select_scan left
hipError_t launch_select_write(const SelectArrays &a, int64_t np, const SelectRule &r, const unsigned long long *prefix,
                               int64_t cap, const SelectOut &out, const SelectPlan &pl, hipStream_t st);
// out.x/v/p/w[k] <- the marker at logical index index[k], k < n: from cur while index[k] < np, from tail beyond; the caller
// has checked 0 <= index[k] < nalloc
hipError_t launch_gather(const SelectArrays &cur, const SelectArrays &tail, int64_t np, const long long *index, int64_t n,
                         const SelectOut &out, hipStream_t st);

// ---- the exact phase-space histogram on a caller's window and grid (kernels_zoom.hip; the definition: include/pic1dp_hip.h
// pic1dp_hip_zoom) ----
constexpr int ZOOM_MAX_BINS = 4096, ZOOM_MAX_CELLS = 1 << 20;
// the window and its grid as the rule takes them (pic1dp_zoom and lx; zoom_fx.cpp zoom_geom fills it on the host, once):
// Lw = x_hi - x_lo, or (x_hi + lx) - x_lo where straddle (x_lo > x_hi); sx = nxb / Lw, sv = nvb / (v_hi - v_lo)
struct ZoomGeom {
  double lx, x_lo, x_hi, v_lo, v_hi, sx, sv;
  int nxb, nvb, straddle;
};
// One pass of pic1dp_hip_zoom over a species' markers (launch_policy.hpp zoom_plan; kernels_zoom.hip k_zoom): the planes
// `planes` (bit 0 markr, 1 total, 2 pertb) of the band of whole v rows [first_row, first_row + rows), one signed 64-bit word
// per (plane, cell) in the workgroup's LDS (lds), or every row straight in memory
struct ZoomPass {
  int blocks, threads;
  bool nt;          // non-temporal marker loads
  size_t bytes;     // dynamic LDS: the band's words where lds, else 0
  bool lds;
  int planes;       // the mask of the pass's planes
  int first_row, rows;
};
constexpr int ZOOM_MAX_PASSES = 64;
struct ZoomPlan {
  int selected;     // planes asked for: 1 ... 3
  int npass;        // 0: arguments out of range
  ZoomPass pass[ZOOM_MAX_PASSES];
};
// The call's device rows.  acc: [planes selected][2][nvb][nxb] -- per plane the hi rows, then the lo rows, the layout the
// limbs are handed out in; rej: [3] terms not summed (2^44 quanta or more, NaN) per plane markr, total, pertb.  Zeroed by the
// caller before a call's passes.  inv_q: 2^-e of total and of pertb (pic1dp_hip_diag_quanta's entries 1 and 2).
struct ZoomArgs {
  long long *acc, *rej;
  double inv_q_p, inv_q_w;
};
hipError_t launch_zoom(const double *x, const double *v, const double *p, const double *w, int64_t np, const ZoomGeom &zg,
                       int which, const ZoomArgs &a, const ZoomPass &ps, int dyn_tail, hipStream_t st);

// ---- the Fourier-Hermite spectrum of the markers (kernels_hermite.hip; the definition: include/pic1dp_hip.h
// pic1dp_hip_hermite) ----
constexpr int HERM_MAX_N = 256, HERM_MAX_COLS = 16, HERM_MAX_MODES = 8;
constexpr int HERM_TILE_LD = 66;   // doubles between two rows of a wave's LDS tile [16][64]: the pad that spreads the fragment reads over the banks
constexpr size_t HERM_WAVE_LDS = sizeof(double) * 2 * 16 * HERM_TILE_LD;   // a wave's two tiles: the columns Y and a block of Psi
// The one pass of a call (launch_policy.hpp hermite_plan; kernels_hermite.hip k_hermite): nb blocks of sixteen Hermite rows
// in every wave's accumulator registers.  partials: the partial sums the launch merges into one output word -- every wave's
// accumulator (into its workgroup's LDS), every workgroup's word (into memory).  blocks = 0: arguments out of range.
struct HermitePlan {
  int blocks, threads;
  bool nt;          // non-temporal marker loads
  size_t bytes;     // dynamic LDS: a wave's two tiles, threads / 64 times
  int nb;           // 4, 8 or 16
  int64_t partials;
};
// The call's constants and device words.  tab: ra[256] then rb[256] (pic1dp_hip_hermite_tables); acc: [16 nb][16] doubles,
// acc[n * 16 + c] the sum of psi_n times column c, zeroed by the caller on the stream.  Column c = (set * nmodes + a) * 2 + t.
struct HermiteArgs {
  const double *tab;
  double *acc;
  double v0, ivt, lx;
  double kk[HERM_MAX_MODES];
  int nmodes, nherm;
};
// ra[n] = 1 / sqrt(n + 1), rb[n] = sqrt(n) / sqrt(n + 1), n < nherm: IEEE sqrt and division, one rounding each (host)
inline void hermite_tables_host(int nherm, double *ra, double *rb) {
  for (int n = 0; n < nherm; ++n) {
    const double s1 = __builtin_sqrt(static_cast<double>(n + 1));
    ra[n] = 1.0 / s1;
    rb[n] = __builtin_sqrt(static_cast<double>(n)) / s1;
  }
}
hipError_t launch_hermite(const double *x, const double *v, const double *p, const double *w, int64_t np, bool with_p, bool with_w,
                          const HermiteArgs &a, const HermitePlan &pl, hipStream_t st);

// ---- marker optimisation events (kernels_opt.hip; host side of the sequential part: optimize.hpp plan_*) ----
// one reference rank block of a species inside the species' packed (tiled) arrays: block-local marker i lies at global
// marker voff + i while i < nvalid0 (the block's valid markers when the event began), else at toff + (i - nvalid0) (its
// tail slots); nvalid0 is the LAYOUT's split point, fixed during an event -- the block's current count travels apart
struct OptBlock {
  double *x, *v, *p, *w;
  int64_t voff, nvalid0, toff;
};
struct OptGrid {
  double lx, v_max;
  int nx, nv;
};
constexpr uint32_t OPT_KEY_IMPORTANT = 0xFFFFFFFFu;
// this block's |delta f|(v) into hist[nv] (device), every bin summed in storage order; synchronises the stream
// scratch: device memory of at least opt_hist_scratch_bytes(np, nv) (the sort's items and temporaries)
size_t opt_hist_scratch_bytes(int64_t np, int nv);
hipError_t opt_hist_block(const OptBlock &b, const OptGrid &g, int64_t np, double *hist, void *scratch, hipStream_t st);
hipError_t opt_merge_keys(const OptBlock &b, const OptGrid &g, const double *hist, double limit, int64_t np, uint32_t *keys,
                          hipStream_t st);
hipError_t opt_remove_vals(const OptBlock &b, const OptGrid &g, const double *hist, double peak, double limit, int by_threshold,
                           int64_t np, uint8_t *skip, double *df, hipStream_t st);
hipError_t opt_split_flags(const OptBlock &b, const OptGrid &g, const double *hist, double limit, int64_t np, uint8_t *flag,
                           hipStream_t st);
// holes[nholes]: the positions below np_new whose marker is gone, ascending (gone: the ids listed, or -- gone_bits
// non-null -- one bit per position); fails when their number is not nholes; scratch: opt_holes_scratch_bytes(np_new)
size_t opt_holes_scratch_bytes(int64_t np_new);
hipError_t opt_holes(const uint32_t *gone_ids, int64_t ngone, const uint32_t *gone_bits, int64_t np_new, int64_t nholes,
                     uint32_t *holes, void *scratch, hipStream_t st);
// scratch: [4 npairs] doubles.  Indices are block-local, 32 bits (a block holds < 2^32 slots)
hipError_t opt_merge_apply(const OptBlock &b, const OptGrid &g, const double *hist, double limit, const uint32_t *dst,
                           const uint32_t *idk, int64_t npairs, const uint32_t *move_pos, const uint32_t *move_id, int64_t nmoves,
                           int64_t ghost, int64_t np_new, double *scratch, hipStream_t st);
hipError_t opt_remove_apply(const OptBlock &b, const OptGrid &g, const double *hist, double peak, double limit, int by_threshold,
                            double keep_scale, const uint32_t *move_pos, const uint32_t *move_id, int64_t nmoves, int64_t ghost,
                            int64_t np_new, hipStream_t st);
hipError_t opt_split_apply(const OptBlock &b, int64_t parents, const uint32_t *ks, const double *dv, int64_t nsplit, int ng, int deltaf,
                           hipStream_t st);
hipError_t opt_copy_segment(const OptBlock &b, int64_t i0, int64_t n, double *dx, double *dv, double *dp, double *dw, int64_t doff,
                            hipStream_t st);

// div_lx's / div_const's algorithm (reciprocal + two FMA corrections) with the host's fma against the true
// quotient on n generated operands: the number of results that differ in any bit (hostcheck.cpp)
int64_t host_div_check(double lx, int nx, uint64_t seed, int64_t n);
// the planners of the GPU marker optimisation against the host routines they restate (optcheck.cpp; test support):
// slots that differ, -1 / -2 when the marker counts / the random streams' positions differ
int64_t host_optimize_check(const pic1dp_input &in, int kind, double threshold, uint64_t seed, int64_t np0, int64_t nalloc,
                            int64_t *np_after);
int64_t host_divc_check(double c, uint64_t seed, int64_t n);
// diag_div's (device_diag.hpp), on the operands of the diagnostics' divisions by lx and 2 v_max
int64_t host_diag_div_check(double lx, int nxo, double vmax, int nvo, uint64_t seed, int64_t n);
// cell index per marker and per-cell counts from (wrapped) x
hipError_t launch_cell_indices(const double *x, int64_t np, const GridConst &g, int32_t *ix,
                               unsigned long long *count, hipStream_t st);

}  // namespace pic1dp
