/*
 * pic1dp_hip.h -- C ABI of the MI355X-native PIC1D time-step engine.
 *
 * This is the drop-in boundary for the hot path of wenjundeng/pic1dp
 * (PIC1D-PETSc): particle push + field gather, charge deposition (+ all-reduce)
 * and the mode-filtered spectral field solve.  The reference has no FFI: the
 * boundary there is three argument-less Fortran module procedures working on
 * module-global PETSc Vecs.  Each entry point below
 * names the reference procedure / call site it replaces (paths relative to the
 * reference tree).  The Fortran side binds these through ISO_C_BINDING
 * (pic1dp_amd/fortran/pic1dp_hip_mod.F90).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - Every function returns int: 0 = success, non-zero = error (the reference's
 *     PetscErrorCode / CHKERRQ convention, src/pic1dp_global.F90:59).
 *     pic1dp_hip_last_error() gives the message of the calling thread's last
 *     failure.
 *   - All state lives in an opaque context created per process/GPU.  Compute
 *     calls enqueue work on the context's HIP stream and return; calls that
 *     hand data to the host (get_*, download, energy, timers) synchronise.
 *   - Called from one host thread per context (the reference is single-threaded
 *     per MPI rank, src/multirand.F90:43-44).
 *   - FP64 everywhere (PetscReal/PetscScalar = real(8)); counts are int64.
 *   - There is NO CPU fallback: without a usable HIP device create() fails.
 */
#ifndef PIC1DP_HIP_H
#define PIC1DP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIC1DP_ABI_VERSION 5
#define PIC1DP_MAX_SPECIES 8
#define PIC1DP_MAX_MODES 4096 /* up to the full spectrum nx/2 of the largest grid */
#define PIC1DP_MAX_INIT_MODES 16
#define PIC1DP_COMM_ID_BYTES 128
#define PIC1DP_XCHG_HANDLE_BYTES 64
#define PIC1DP_MAX_OPT 32

/* error codes */
enum {
  PIC1DP_OK = 0,
  PIC1DP_ERR_ARG = 1,      /* bad argument / unsupported parameter value */
  PIC1DP_ERR_HIP = 2,      /* HIP runtime failure (message has the HIP error) */
  PIC1DP_ERR_NODEVICE = 3, /* no usable gfx950 device: no CPU fallback exists */
  PIC1DP_ERR_STATE = 4,    /* call out of sequence (e.g. step before load) */
  PIC1DP_ERR_COMM = 5,     /* RCCL failure / library not loadable */
  PIC1DP_ERR_RNG = 6,      /* multirand self-test failed or would hang */
  PIC1DP_ERR_NOMEM = 7
};

/* Run-time mirror of the compile-time parameters of src/pic1dp_input.F90:32-256.
 * Field names are the reference names without the "input_" prefix. */
typedef struct pic1dp_input {
  int32_t abi_version;          /* must be PIC1DP_ABI_VERSION */
  int32_t ntime_max;            /* :32 */
  int32_t linear;               /* :43  0 nonlinear, 1 linear */
  int32_t iptcldist;            /* :54  0 Maxwellian 1 two-stream1 2 two-stream2 3 bump-on-tail */
  int32_t nspecies;             /* :57 */
  int32_t nmode;                /* :75 */
  int32_t init_nmode;           /* :87 */
  int32_t deltaf;               /* :106 0 full-f, 1 delta-f */
  int32_t imarker;              /* :122 1 physical, 2 uniform in v */
  int32_t nx;                   /* :128 */
  int32_t nv;                   /* :131 (header of pic1dp.out only) */
  int32_t iptclshape;           /* :138 only 4 (on-the-fly linear shape) is built */
  int32_t nx_opd;               /* :253 */
  int32_t nv_opd;               /* :256 */
  int32_t multirand_al_int;     /* :217 */
  int32_t multirand_seed_type;  /* :223 */
  int32_t multirand_warmup;     /* :226 */
  int32_t multirand_selftest;   /* :233 */
  int64_t nparticle_max;        /* :113 global allocation per species */
  int64_t species_nparticle_init[PIC1DP_MAX_SPECIES]; /* :116 */
  double time_max;              /* :35 */
  double lx;                    /* :46 */
  double dt;                    /* :109 */
  double v_max;                 /* :125 */
  double output_interval;       /* :250 */
  double species_charge[PIC1DP_MAX_SPECIES];       /* :67 */
  double species_mass[PIC1DP_MAX_SPECIES];         /* :68 */
  double species_temperature[PIC1DP_MAX_SPECIES];  /* :69 */
  double species_temperature2[PIC1DP_MAX_SPECIES]; /* :70 */
  double species_density[PIC1DP_MAX_SPECIES];      /* :71 */
  double species_v0[PIC1DP_MAX_SPECIES];           /* :72 */
  int32_t modes[PIC1DP_MAX_MODES];                 /* :79 */
  int32_t init_mode[PIC1DP_MAX_INIT_MODES];        /* :90 */
  double init_mode_cos[PIC1DP_MAX_INIT_MODES];     /* :97 */
  double init_mode_sin[PIC1DP_MAX_INIT_MODES];     /* :98 */
  /* marker optimisation, :141-206 (all counts 0 = disabled, the default) */
  int32_t nmerge;               /* :146 */
  int32_t nremove;              /* :162 */
  int32_t nsplit;               /* :188 */
  int32_t typeremove;           /* :172 1 threshold + fraction, 2 by the |delta f| profile */
  int32_t split_ngroup;         /* :203 */
  int32_t reserved0;
  double remove_frac;           /* :184 */
  double split_dv_sig_frac;     /* :206 */
  double tmerge[PIC1DP_MAX_OPT];      /* :149 ascending */
  double thshmerge[PIC1DP_MAX_OPT];   /* :155 */
  double tremove[PIC1DP_MAX_OPT];     /* :165 */
  double thshremove[PIC1DP_MAX_OPT];  /* :177 */
  double tsplit[PIC1DP_MAX_OPT];      /* :191 */
  double thshsplit[PIC1DP_MAX_OPT];   /* :197 */
} pic1dp_input;

/* Placement of this process in the particle decomposition.
 * The reference splits every particle Vec into `npe` contiguous PETSC_DECIDE
 * blocks (src/pic1dp_particle.F90:89-94,129) and seeds one RNG stream per MPI
 * rank (:159-160).  Here `npe` is the number of REFERENCE ranks being
 * reproduced; this process (rank of nranks, one per GPU) owns the contiguous
 * group of npe/nranks reference blocks starting at rank*npe/nranks, so a
 * 1-GPU run can reproduce an 8-rank reference run ("virtual ranks").
 * npe must be a multiple of nranks; npe = nranks gives the plain mapping. */
typedef struct pic1dp_layout {
  int32_t rank;    /* global_mype of this process, 0-based */
  int32_t nranks;  /* processes = GPUs in the job */
  int32_t npe;     /* reference ranks reproduced (global_npe); 0 -> nranks */
  int32_t device;  /* HIP device ordinal; -1 -> rank % device count */
} pic1dp_layout;

typedef struct pic1dp_ctx pic1dp_ctx; /* opaque */

/* wall-clock timer ids: the reference's ids, src/pic1dp_global.F90:38-50 */
enum {
  PIC1DP_IWT_TOTAL = 1,
  PIC1DP_IWT_INIT = 2,
  PIC1DP_IWT_PARTICLE_LOAD = 3,
  PIC1DP_IWT_PUSH_PARTICLE = 4,
  PIC1DP_IWT_PARTICLE_SHAPE = 5,
  PIC1DP_IWT_COLLECT_CHARGE = 6,
  PIC1DP_IWT_FIELD_ELECTRIC = 7,
  PIC1DP_IWT_PARTICLE_OPTIMIZE = 8,
  PIC1DP_IWT_OUTPUT = 9,
  PIC1DP_IWT_FINAL = 10,
  PIC1DP_IWT_MPIALLREDU = 21,
  PIC1DP_IWT_SCATTER = 22
};

/* ---- library ---------------------------------------------------------- */
int pic1dp_hip_abi_version(void);
const char *pic1dp_hip_last_error(void);
/* 1 when the library is a -DPIC1DP_TUNING build (it then also reads the measurement knobs of
 * tools/README.md from the environment), 0 for the product build, which compiles none of them */
int pic1dp_hip_tuning_build(void);
/* number of visible HIP devices (0 when none; never fails) */
int pic1dp_hip_device_count(void);
/* fill `in` with the values of the reference's input file
 * (src/pic1dp_input.F90), except multirand_seed_type = 1 (reproducible) */
int pic1dp_hip_input_defaults(pic1dp_input *in);

/* sizeof(pic1dp_input) as the library was compiled: lets a binding in another
 * language verify its struct layout before the first call */
int pic1dp_hip_input_size(void);
/* the two validity checks of input_init (src/pic1dp_input.F90:287-308) plus the
 * range checks of this build, without touching a device */
int pic1dp_hip_input_validate(const pic1dp_input *in, const pic1dp_layout *layout);

/* ---- host-only helpers (no device needed) --------------------------------
 * allocated slots / valid markers of reference block `mype` of `npe`
 * (src/pic1dp_particle.F90:129, :240-248) */
int pic1dp_hip_block_sizes(const pic1dp_input *in, int32_t ispecies, int32_t mype,
                           int32_t npe, int64_t *nalloc, int64_t *np);
/* particle_load of ONE reference block into HOST arrays: x, v, p, w each hold
 * nspecies * nalloc doubles, species-major (species s at offset s*nalloc).
 * This is the generator pic1dp_hip_particle_load uses before the upload. */
int pic1dp_hip_host_particle_load(const pic1dp_input *in, int32_t mype, int32_t npe,
                                  double *x, double *v, double *p, double *w,
                                  int64_t nalloc);

/* n raw 64-bit draws (multirand_int64, as two's-complement int64) of the
 * loader's generator after multirand_init(al_int, seed_type, mype, warmup,
 * selftest) -- src/multirand.F90:132-383; lets a host or a test check the
 * stream against the reference's */
int pic1dp_hip_host_multirand_int64(int32_t al_int, int32_t seed_type, int32_t mype,
                                    int32_t warmup, int32_t selftest, int64_t *out,
                                    int64_t n);

/* ---- life cycle -------------------------------------------------------
 * create  <-> input_init + particle_init + field_init
 *             (src/pic1dp.F90:57-59; src/pic1dp_particle.F90:66-139;
 *              src/pic1dp_field.F90:55-212)
 * destroy <-> particle_final + field_final (src/pic1dp.F90:113-114) */
int pic1dp_hip_create(const pic1dp_input *in, const pic1dp_layout *layout,
                      pic1dp_ctx **out);
int pic1dp_hip_destroy(pic1dp_ctx *ctx);

/* local sizes of this process: allocated slots (sum of its reference blocks'
 * PETSC_DECIDE sizes) and valid markers particle_np (src/pic1dp_particle.F90:54,
 * :240-248) of one species */
int pic1dp_hip_local_sizes(pic1dp_ctx *ctx, int32_t ispecies, int64_t *nalloc,
                           int64_t *np);

/* ---- initial condition -------------------------------------------------
 * particle_load (src/pic1dp_particle.F90:145-269) with multirand
 * (src/multirand.F90): native host loader, one RNG stream per owned reference
 * block (seeded with that block's mype), then H2D.  Uses the multirand_*
 * fields of the input. */
int pic1dp_hip_particle_load(pic1dp_ctx *ctx);
/* Members of an ENSEMBLE of otherwise identical runs: reference block b of the next
 * particle_load draws from the stream multirand_init(..., mype = b + offset, ...)
 * instead of mype = b (src/pic1dp_particle.F90:159-160).  offset 0 (default) is the
 * reference's constant-seed run (seed_type 1) the parity tests are about; the
 * reference itself gets its ensembles from seed_type 2 / 3 (clock, /dev/urandom:
 * src/multirand.F90:291-306) and compares their growth rates (tools/runinfo.py:
 * 94-122,136-231) -- this is the reproducible form of that.  Block sizes, weights
 * and everything else are those of the npe-rank load. */
int pic1dp_hip_set_seed_offset(pic1dp_ctx *ctx, int32_t offset);
/* The initial condition made ON THE DEVICE: one streaming kernel pass per species writes x, v, p, w of
 * every slot, nothing crosses PCIe and no sequential stream is drawn.  A marker is a function of its GLOBAL index alone:
 * valid slot i of species s is global marker g = G0_s + i, G0_s = the valid markers of the reference blocks before the
 * first one this process owns (pic1dp_hip_load_origin), so a run has the same markers whatever npe and nranks are.
 *   mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31 (mod 2^64)
 *   kind 1, counter-based random: key = mix64(0x7069633164704C44 + 256 seed_offset + s), r(c) = mix64(key + (c + 1)
 *     0x9E3779B97F4A7C15), u_v = (r(2g) >> 11) 2^-53, u_x = (r(2g + 1) >> 11) 2^-53   (seed_offset: set_seed_offset);
 *   kind 2, quiet start: u_v = (bitrev64(g) >> 11) 2^-53, the base-2 radical inverse; u_x = R3(g) / 3^21, R3 the
 *     reversal of the 21 base-3 digits of g, one IEEE division.  The same sequence for every species.  It needs
 *     species_nparticle_init <= 3^21 = 10 460 353 203 and seed offset 0.
 * Marker values: the imarker = 2 branch of particle_load in its operation order -- v = (u_v - 0.5) 2 v_max, p from the
 * iptcldist formula (exp: the kernels' table-driven exp, within 1 ulp of libm), x = u_x lx, w = amp p with amp the sum
 * over init_mode of cos, sin (the device's sincos), p += w in a nonlinear run.  Tail slots [np, nalloc) hold +0.0.
 * The context is left as pic1dp_hip_particle_load leaves it (counts, optimisation counters, every owned block's
 * generator initialised with no draw consumed, time 0, empty energy history).
 * PIC1DP_ERR_ARG, with the context untouched: kind not 1 or 2; imarker = 1; kind 2 with a seed offset or with more than
 * 3^21 markers of a species. */
int pic1dp_hip_particle_load_device(pic1dp_ctx *ctx, int32_t kind);
/* host only: G0 of species `ispecies` for the process `layout` describes (rank, nranks, npe; null: one rank, one block) */
int pic1dp_hip_load_origin(const pic1dp_input *in, const pic1dp_layout *layout, int32_t ispecies, int64_t *g0);
/* host only: u_v and u_x of the global markers g0 ... g0 + n - 1 of a species, as defined above (uv, ux: n doubles each).
 * PIC1DP_ERR_ARG: kind not 1 or 2, ispecies outside [0, PIC1DP_MAX_SPECIES), seed_offset < 0 (as set_seed_offset), g0 < 0,
 * kind 2 with seed_offset != 0 or g0 + n > 3^21 */
int pic1dp_hip_host_load_uniforms(int32_t kind, int32_t seed_offset, int32_t ispecies, int64_t g0, int64_t n, double *uv,
                                  double *ux);
/* alternative for a host that ran the reference's own particle_load:
 * hand over HOST arrays of one species (n = allocated slots, np = valid) --
 * the VecGetArrayF90 view of particle_x/v/p/w (src/pic1dp_particle.F90:34-36) */
int pic1dp_hip_particles_upload(pic1dp_ctx *ctx, int32_t ispecies,
                                const double *x, const double *v,
                                const double *p, const double *w, int64_t n,
                                int64_t np);
/* copy the current particle_x/v/p/w of one species back to HOST arrays of
 * n = allocated slots (any pointer may be NULL) */
int pic1dp_hip_particles_download(pic1dp_ctx *ctx, int32_t ispecies, double *x,
                                  double *v, double *p, double *w, int64_t n);
/* RK backups particle_x_bak/v_bak/w_bak as the reference would hold them
 * (valid between push(1) and the end of push(2)) */
int pic1dp_hip_particles_download_bak(pic1dp_ctx *ctx, int32_t ispecies,
                                      double *xb, double *vb, double *wb,
                                      int64_t n);

/* ---- the hot path ------------------------------------------------------ */
/* interaction_collect_charge, iptclshape 4 (src/pic1dp_interaction.F90:79-151,
 * call sites src/pic1dp.F90:71,88): periodic wrap of x (stored back), linear
 * deposit, species charge scaling, all-reduce over ranks (RCCL), normalisation
 * into field_chargeden.  The last step (on one rank: the species sum too) runs in
 * the launch of the solve_field that follows, or as soon as anything else asks for
 * field_chargeden or touches the accumulators (one launch less per sub-step: at the
 * reference's default size a launch is 5 % of a step); PIC1DP_LAZY_CALLS=0: at once */
int pic1dp_hip_collect_charge(pic1dp_ctx *ctx);
/* field_solve_electric (src/pic1dp_field.F90:218-270, call sites
 * src/pic1dp.F90:72,89): mode-filtered partial DFT solve of field_chargeden
 * into field_electric, field_mode_re, field_mode_im */
int pic1dp_hip_solve_field(pic1dp_ctx *ctx);
/* interaction_push_particle (src/pic1dp_interaction.F90:161-370, call site
 * src/pic1dp.F90:80); irk = global_irk = 1 or 2.
 * In the reference's sequence push(1), collect_charge, solve_field, push(2),
 * collect_charge, solve_field the push is only noted and the collect_charge
 * that follows runs one whole-step kernel for both; from the second step on the
 * collect_charge after push(1) touches no marker at all -- the previous step's
 * kernel has predicted its charge -- so a step is ONE pass over
 * the markers (56 instead of 184 bytes per marker and step), and on one rank the
 * solve_field after the second collect_charge solves both fields of the step in one
 * launch: two launches per time step.  Whatever looks at the markers in between first gets the
 * ordinary kernels run, so every observable state is the eager one, bit for
 * bit.  PIC1DP_LAZY_CALLS=0 in the environment: one kernel per call, at once. */
int pic1dp_hip_push(pic1dp_ctx *ctx, int32_t irk);
/* particle_optimize (src/pic1dp_particle.F90:724-783; call site src/pic1dp.F90:82,
 * right after the push of sub-step irk): when global_time + dt has reached the
 * next entry of tmerge / tremove / tsplit and irk == 2, runs particle_merge /
 * particle_remove / particle_split (:411-715) on every owned reference block and
 * sets *flag_optimized = 1.  The markers stay on the device: the |delta f|(v)
 * histogram is folded there in the reference's order of additions, one small key per
 * marker (1-8 B) goes to the host, which walks the keys exactly as these sequential
 * routines walk the markers (visiting order, swap-with-last, the block's random
 * stream; the blocks side by side on host threads), and the decisions are applied on
 * the device (PIC1DP_OPT_HOST=1: the pass on host copies of the
 * markers, kept as the cross-check).  Off the timed path and disabled by default.  pic1dp_hip_step calls
 * this itself.  Needs markers loaded by pic1dp_hip_particle_load (the blocks'
 * generators continue from the load), delta-f only like the reference. */
int pic1dp_hip_particle_optimize(pic1dp_ctx *ctx, int32_t irk, int32_t *flag_optimized);
/* one Runge-Kutta sub-step = push(irk); [particle_optimize;] collect_charge;
 * solve_field (src/pic1dp.F90:80-89) with push+wrap+deposit fused into one kernel */
int pic1dp_hip_substep(pic1dp_ctx *ctx, int32_t irk);
/* nsteps time steps: {substep(1); substep(2); itime += 1; time += dt}
 * (src/pic1dp.F90:79-93).  The field energy int E^2 dx after every step is
 * appended to a device-side history (see pic1dp_hip_energy_history). */
int pic1dp_hip_step(pic1dp_ctx *ctx, int32_t nsteps);
/* how pic1dp_hip_step advances a time step (marker pushes are bit-identical given
 * identical fields; only the memory traffic differs):
 *   0 (default) whole-step kernels: the half-step state is recomputed in the
 *     second sub-step instead of being stored and re-read, state updated in place;
 *     from the second step on ONE pass over the markers per step (the second
 *     sub-step's kernel also deposits the next first sub-step's charge as
 *     coefficients of the kept field modes: 56-72 B per marker per step; the
 *     half-step charge then equals a marker-by-marker deposit up to rounding;
 *     PIC1DP_PREDICT=0 in the environment keeps the two passes, 88 B).  The
 *     prediction is held as LDS tiles (two kept modes; nx up to ~1700) or, with
 *     one kept mode (nx up to ~5000), as six
 *     sums over the markers -- then, through the call sites, the collect_charge after push(1)
 *     leaves in field_chargeden the kept mode's content of the half-step charge
 *     density only (all that solve_field looks at; nothing in the reference driver
 *     reads it there).  A host that DOES read it there gets the reference's vector:
 *     see pic1dp_hip_get_field.
 *     Falls back to two passes otherwise, and to mode 1 when nx is too large for
 *     three grid tiles in LDS
 *   1 two fused sub-steps through the RK ping-pong sets (136 B per marker) */
int pic1dp_hip_set_step_mode(pic1dp_ctx *ctx, int32_t mode);
/* how step mode 0 predicts the next first sub-step's charge for this input: 0 not at
 * all (two passes per step), 1 prediction tiles (k_step_one), 2 six sums (k_step_sums) */
int pic1dp_hip_predict_kind(pic1dp_ctx *ctx, int32_t *kind);
/* Diagnostics of output_all taken inside the time step that precedes it.  A step after which the
 * driver will call output_all (the cadence test of src/pic1dp.F90:98-107 evaluated one step ahead
 * from the library's time, see set_time; the last step of a pic1dp_hip_step call, or the
 * collect_charge that follows push(2)) can take the histograms of output_ptcldist and the kinetic
 * sums of output_field inside its marker kernel, on the state it has just computed
 * (k_step_full<DIAG>): pic1dp_hip_output_scalars / pic1dp_hip_ptcldist then cost no pass over the
 * markers.  Results equal the separate pass up to the summation order of the atomics.
 * Cost at 1e8 markers: inside a two-pass step +0.17 ms an output (the histograms as 64-bit
 * fixed-point sums in the LDS; +0.48 as double sums, +0.6 as a pass of its own).
 *   on = 0 (default): never -- a host that never asks for output would pay ~20 % on that launch;
 *   on = 1: where it pays.  Not on a predicted one-pass step (pic1dp_hip_predict_kind != 0):
 *           k_step_full<DIAG> cannot predict the next step's half-step charge, so the step after
 *           the output would run a first-sub-step pass again; there the step stays k_step_one and
 *           the diagnostics take their own pass (32 B per marker) when output_all asks for them;
 *   on = 2: always. */
int pic1dp_hip_set_output_fusion(pic1dp_ctx *ctx, int32_t on);
/* which field solve pic1dp_hip_solve_field / substep / step perform:
 *   0 (default) the reference's field_solve_electric: mode-filtered partial DFT
 *     (src/pic1dp_field.F90:218-270) -- the only solver with reference parity
 *   1 opt-in alternative, NOT in the reference: second-order finite differences
 *     keeping all modes, -phi'' = rho - <rho> as a tridiagonal system solved by
 *     parallel cyclic reduction on the GPU, E = -dphi/dx by central differences
 *     (3 <= nx <= 4096).  field_mode_re/im still hold the kept modes of the
 *     mode-filter solve. */
int pic1dp_hip_set_field_solver(pic1dp_ctx *ctx, int32_t kind);
/* how the mode-filter solve (solve_field, substep, step; also the kept modes that field solver 1 still reports)
 * computes the DFT of field_chargeden -- opt-in, per context:
 *   0 (default) the direct partial DFT against dense cos / -sin tables: the reference's rounding and, with a
 *     layout of npe ranks, its npe-rank summation order
 *   1 an FFT: for each kept mode m, bin b = m mod nx of a mixed-radix (2, 3, 4, 5) FFT gives R + i I, and
 *     mode_re = I / nx * grad_inv, mode_im = -R / nx * grad_inv as in transform 0; E = 2 sum_m (mode_re cos -
 *     mode_im sin)(2 pi m ix / nx) by the inverse FFT of the Hermitian spectrum.  Twiddles from exactly reduced
 *     angles.  Independent of npe.  Relative error against the exact sums ~1e-15.  Transform 1 runs none of the
 *     one-pass (predicted) or fused paths: step mode 0 takes two passes per step -- it is meant for many kept modes.
 * Supported nx for transform 1: nx = 2^a 3^b 5^c with 2 <= nx <= 8192, odd nx only up to 3375.  Any other transform,
 * or an unsupported nx, returns PIC1DP_ERR_ARG.  Switching while the half-step field of a call-site pair waits to be
 * adopted deposits the half-step charge for real instead (as set_field_solver). */
int pic1dp_hip_set_field_transform(pic1dp_ctx *ctx, int32_t transform);
/* *supported = 1 if the given transform handles nx, else 0 (host only, no device, no context) */
int pic1dp_hip_field_transform_supported(int32_t nx, int32_t transform, int32_t *supported);
/* field_electric as it was between the two sub-steps of the last time step
 * taken by pic1dp_hip_step ([nx]) */
int pic1dp_hip_get_field_half(pic1dp_ctx *ctx, double *electric_half);
/* wait for everything enqueued on the context's stream */
int pic1dp_hip_sync(pic1dp_ctx *ctx);

/* global_itime / global_time (src/pic1dp_global.F90:62-63) */
int pic1dp_hip_get_time(pic1dp_ctx *ctx, int32_t *itime, double *time);
int pic1dp_hip_set_time(pic1dp_ctx *ctx, int32_t itime, double time);
/* check_termination (src/pic1dp.F90:133-148): *flag = 1 to terminate */
int pic1dp_hip_check_termination(pic1dp_ctx *ctx, int32_t *flag);
/* output cadence test of src/pic1dp.F90:98-106 evaluated at the current time */
int pic1dp_hip_output_due(pic1dp_ctx *ctx, int32_t itermination, int32_t *flag);
/* how many iterations of the driver loop (src/pic1dp.F90:78-109) lie between the current counters and the next
 * output_all -- the cadence test of :98-106 and check_termination (:133-148) evaluated ahead, step by step, with
 * the very additions the loop makes (time = time + dt).  A host that hands the whole irk loop to
 * pic1dp_hip_step can ask for exactly that many steps in one call and loses no record: *nsteps >= 1 while the run
 * has not terminated, 0 once it has. */
int pic1dp_hip_steps_to_output(pic1dp_ctx *ctx, int32_t *nsteps);

/* ---- field access (what output_field reads, src/pic1dp_output.F90:173-186) */
/* any pointer may be NULL; E, chargeden: [nx]; mode_re, mode_im: [nmode].
 * HALF-STEP CHARGE DENSITY -- the one place where the state a host can look at differs
 * from what the reference would hold: between the collect_charge after push(1) and the
 * next collect_charge, when that half-step charge was predicted as six sums
 * (pic1dp_hip_predict_kind = 2: one kept mode), field_chargeden
 * holds its kept mode's content only.  Asking for chargeden here rebuilds the whole
 * vector on a one-rank context: the half-step state is pushed into memory after all and
 * deposited (that step then runs as two ordinary sub-steps -- a noted push(2) is run at
 * once as well; results unchanged to rounding).  On several ranks the rebuild would need
 * the charge sum -- a collective an inspection on one rank must not start -- so there
 * chargeden keeps the kept mode's content between the sub-steps; a host that needs the
 * full half-step vector on several ranks calls pic1dp_hip_set_step_mode(ctx, 1) or sets
 * PIC1DP_PREDICT=0.  Whether the vector handed out is the reference's or the kept mode's
 * content is never left to guessing: pic1dp_hip_chargeden_state says which.  Pass
 * chargeden = NULL to leave it alone. */
int pic1dp_hip_get_field(pic1dp_ctx *ctx, double *electric, double *chargeden,
                         double *mode_re, double *mode_im);
/* *kept_mode_only = 1: field_chargeden (as pic1dp_hip_get_field hands it out now) holds
 * only the kept mode's content of the half-step charge density -- the rebuild described
 * above was not possible (several ranks; or the markers have been moved on since by
 * calls outside the push / collect_charge / solve_field sequence); 0: it is the vector
 * the reference holds (src/pic1dp_interaction.F90:138-150). */
int pic1dp_hip_chargeden_state(pic1dp_ctx *ctx, int32_t *kept_mode_only);
/* overwrite field_electric (testing the push against a prescribed field) */
int pic1dp_hip_set_electric(pic1dp_ctx *ctx, const double *electric);
/* overwrite field_chargeden (testing the solve; field_test of
 * src/pic1dp_field.F90:276-309) */
int pic1dp_hip_set_chargeden(pic1dp_ctx *ctx, const double *chargeden);
/* int E^2 dx = ||E||_2^2 * lx / nx (src/pic1dp_output.F90:120-124) */
int pic1dp_hip_field_energy(pic1dp_ctx *ctx, double *energy);
/* energies recorded by step(): copies min(count, max) values, oldest first */
int pic1dp_hip_energy_history(pic1dp_ctx *ctx, double *energy, int64_t max,
                              int64_t *count);
int pic1dp_hip_energy_history_reset(pic1dp_ctx *ctx);
/* per-species sums of output_field (src/pic1dp_output.F90:126-172), local to
 * this process: out[0]=sum v^2, out[1]=sum v^2 p, out[2]=sum v^2 w */
int pic1dp_hip_energy_sums(pic1dp_ctx *ctx, int32_t ispecies, double out[3]);
/* cell index ix of every valid marker of one species and the per-cell marker
 * counts, as the deposit computes them (src/pic1dp_interaction.F90:106-107);
 * ix: [np] int32, count: [nx] int64, either may be NULL */
int pic1dp_hip_cell_indices(pic1dp_ctx *ctx, int32_t ispecies, int32_t *ix,
                            int64_t *count);

/* ---- diagnostics of output_all (called every output_interval, not timed) --
 * realbuf of output_field (src/pic1dp_output.F90:117-175): out[0] = time,
 * out[1] = int E^2 dx, then per species s: out[2+3s] = sum v^2,
 * out[3+3s] = total kinetic sum, out[4+3s] = perturbed kinetic sum (the linear /
 * full-f adjustments of :152-170 applied).  n must be 2 + 3*nspecies.  Sums are
 * all-reduced over ranks when a communicator exists.
 * energy_sums, output_scalars and ptcldist share one pass over a species'
 * markers (histograms and kinetic sums together); its results are kept until a
 * call changes the markers, so the sequence of output_all costs one pass. */
int pic1dp_hip_output_scalars(pic1dp_ctx *ctx, double *out, int32_t n);
/* (x,v) and v distributions of output_ptcldist (src/pic1dp_output.F90:196-477)
 * of one species, computed on the GPU: markr/total/pertb_xv hold
 * nx_opd*nv_opd doubles (index iv*nx_opd+ix), markr/total/pertb_v hold nv_opd.
 * finish = 0: this rank's raw sums (:239-315).
 * finish = 1: what the reference writes: summed over ranks (when a communicator
 *             exists), linear total += pertb (:328-331), scaled by the grid
 *             sizes (:361-369) and, for full-f, pertb = total - f0 (:370-453). */
int pic1dp_hip_ptcldist(pic1dp_ctx *ctx, int32_t ispecies, int32_t finish,
                        double *markr_xv, double *total_xv, double *pertb_xv,
                        double *markr_v, double *total_v, double *pertb_v);

/* output_all in ONE call (src/pic1dp_output.F90:100-189, 196-477; call sites src/pic1dp.F90:74,107): what
 * pic1dp_hip_output_scalars, pic1dp_hip_get_field and pic1dp_hip_ptcldist(finish = 1) of every species hand out,
 * with the diagnostics passes and every transfer enqueued together and ONE wait (the separate calls wait
 * three times and more per record).  scalars: [2 + 3 nspecies]; electric, chargeden: [nx]; mode_re, mode_im:
 * [nmode]; dist: [nspecies][3 nx_opd nv_opd + 3 nv_opd] = markr_xv | total_xv | pertb_xv | markr_v | total_v |
 * pertb_v of each species in turn.  Any pointer but scalars may be NULL.  On several ranks the call composes the
 * separate ones (RCCL communicator: they reduce; no communicator: an error, as pic1dp_hip_ptcldist).
 * When the call may come: anywhere in a time step (a noted push becomes memory first; chargeden is field_chargeden as it
 * stands, the kept mode's content only where pic1dp_hip_chargeden_state says so) but not between charge_local and
 * charge_reduced: PIC1DP_ERR_STATE there, nothing written, the pending deposit untouched. */
int pic1dp_hip_output_all(pic1dp_ctx *ctx, double *scalars, int32_t nscalars, double *electric, double *chargeden,
                          double *mode_re, double *mode_im, double *dist);
/* ---- split-phase diagnostics for a host that owns the reductions (MPI) ----
 * output_all sums its diagnostics over the ranks (VecSum / MPI_Reduce, src/pic1dp_output.F90:126-151,333-356).
 * With an RCCL communicator output_scalars and ptcldist(finish = 1) do that themselves; a host with its own
 * MPI takes the local sums -- pic1dp_hip_energy_sums per species, pic1dp_hip_ptcldist(finish = 0) --, reduces
 * them to its rank 0 and hands the sums back:
 *   output_scalars_from: sums[3*nspecies] = sum v^2, sum v^2 p, sum v^2 w per species, summed over ranks ->
 *     out[2 + 3*nspecies] as pic1dp_hip_output_scalars writes it (time, int E^2 dx, three energies per
 *     species, :152-170)
 *   ptcldist_finish: the six raw histograms summed over ranks -> what the reference writes (:328-331,
 *     :361-453), in place */
int pic1dp_hip_output_scalars_from(pic1dp_ctx *ctx, const double *sums, double *out, int32_t n);
int pic1dp_hip_ptcldist_finish(pic1dp_ctx *ctx, int32_t ispecies, double *markr_xv, double *total_xv,
                               double *pertb_xv, double *markr_v, double *total_v, double *pertb_v);

/* ---- split-phase deposit for a host that owns the reduction (MPI) ------
 * charge_local: everything of collect_charge up to the all-reduce
 *   (src/pic1dp_interaction.F90:81-128) -> this rank's charge2[nx] on the host
 * charge_reduced: hand back the globally summed array; finishes :138-150
 * The array is to be summed element by element over the ranks and handed back whole:
 * after a noted push(1) whose charge the previous step has predicted as six sums
 * (pic1dp_hip_predict_kind = 2) it carries those sums in its first six elements and
 * zeros behind, not a charge vector. */
int pic1dp_hip_charge_local(pic1dp_ctx *ctx, double *charge2);
int pic1dp_hip_charge_reduced(pic1dp_ctx *ctx, const double *charge1);

/* ---- exact charge sum (round 7; opt-in) ----------------------
 * set_charge_sum(kind): 0 FP64 atomics (the reference's sum; default), 1 exact.  In kind 1 every contribution
 * wl q, (1 - wl) q of the deposit (src/pic1dp_interaction.F90:110,113) is rounded once to a whole number of quanta
 * 2^e_s of its species, and the integers are summed exactly -- in the LDS, across workgroups, across ranks (RCCL
 * int64, the one-hop exchange, or the host through the calls below).  Each species' total is converted to double
 * once (round to nearest even) and times 2^e_s; from there the FP64 path runs as in kind 0 (species sum, nx/lx, the
 * full-f -Z n0).  chargeden, E, the kept modes and the energy history then have the same bits whatever the launch
 * shape, step mode, call sites (eager or lazy), reduction, or split of the markers over ranks.
 *   - Only between time steps (nothing noted or owed, no charge_local pending): PIC1DP_ERR_STATE otherwise.  All ranks
 *     switch at the same point of the run.  Back to 0 restores kind 0's paths.
 *   - Kind 1 predicts nothing: step mode 0 runs two passes per step (pic1dp_hip_predict_kind reports 0 while it is
 *     set), and the diagnostics of output_all are taken in their own pass with their own summation (exact on
 *     request as well: pic1dp_hip_set_diag_sum below).
 *   - A contribution of 2^62 quanta or more (a weight ~2^10 past the input's bound) is not summed: it is counted
 *     (kernel_stats which = 14) and the next synchronising call returns PIC1DP_ERR_ARG naming the species.
 *   - charge_local / charge_reduced return PIC1DP_ERR_STATE in kind 1 (a sum of doubles cannot be exact).
 * charge_quantum: e_s = ceil(log2 B_s) - 52, B_s a bound on the species' |p| and |w| from the input alone (the
 *   loader's prefactor times the distribution's peak times 1 + sum |perturbation amplitudes|): every rank agrees
 *   without a collective.  Touches no device. */
int pic1dp_hip_set_charge_sum(pic1dp_ctx *ctx, int32_t kind);
int pic1dp_hip_charge_quantum(const pic1dp_input *in, int32_t ispecies, int32_t *log2_quantum);
/* split phase of kind 1 for a host that owns the reduction (MPI_Allreduce of MPI_INT64_T with MPI_SUM):
 * charge_local_exact -> limbs[nspecies][2][nx] int64: for species s and cell i, hi = limbs[(2 s) nx + i] and
 *   lo = limbs[(2 s + 1) nx + i], 0 <= lo < 2^32; the cell's total is (hi 2^32 + lo) quanta 2^e_s.
 * charge_reduced_exact <- the same array summed element by element over the ranks (lo need not be normalised). */
int pic1dp_hip_charge_local_exact(pic1dp_ctx *ctx, int64_t *limbs);
int pic1dp_hip_charge_reduced_exact(pic1dp_ctx *ctx, const int64_t *limbs);

/* ---- exact sums for the diagnostics of output_all (opt-in) -----------------
 * set_diag_sum(kind): 0 the pass as it was (FP64 sums, or fixed point scaled per pass; default), 1 exact.  In kind 1
 * energy_sums, output_scalars, ptcldist(finish = 0 / 1) and output_all are fixed by the input and the markers alone:
 * they do not depend on launch shape, storage order of the markers, split over ranks or API path.
 *   Terms.  Per species the float64 products of the pass, in the reference's order: for a marker with |v| < v_max the
 *     four corner weights sx sv, sx (1 - sv), (1 - sx) sv, (1 - sx)(1 - sv), each times 1, p and w (planes markr,
 *     total, pertb; full-f: no pertb terms), with the two edge rules of DESIGN 2.1; for every marker slot the kinetic
 *     sums count (the tail slots included) v v, (v v) p, (v v) w.
 *   Quanta.  Every term t becomes n = rint(t 2^-e), one rounding to nearest even; the integers are summed exactly -- in
 *     registers, in the LDS, across workgroups and across ranks --, every bin's total is converted to double once
 *     (round to nearest even) and multiplied by 2^e.  From that double on the finish runs as in kind 0.
 *   v histograms.  The exact integer sums over ix of the (x, v) planes' bins, on every path.
 *   diag_quanta: the six e of a species -- markr, total, pertb, sum v^2, sum v^2 p, sum v^2 w -- from the input alone
 *     (no device): with kb = ceil(log2 B_s) (B_s: charge_quantum's bound) and kv = ceil(log2 v_max^2),
 *     -40, kb - 40, kb - 40, kv - 52, kv + kb - 52, kv + kb - 52.
 *   A histogram term of 2^44 quanta or more, a kinetic term of 2^62 or more (|p|, |w| 2^4 past the bound; |v| beyond
 *     32 v_max), or a NaN is not summed: it is counted (kernel_stats which = 15) and every call that hands out
 *     diagnostics of that pass returns PIC1DP_ERR_ARG naming the species and the plane, until the markers change.
 *   - Only between time steps, as set_charge_sum (PIC1DP_ERR_STATE otherwise); independent of the charge sum's kind.
 *     The switch drops the cached diagnostics.
 *   - Kind 1 always takes the diagnostics in their own pass: set_output_fusion is ignored while it is set, and the
 *     one-pass prediction survives an output_all as it does in kind 0.
 *   - With an RCCL communicator output_scalars, ptcldist(finish = 1) and output_all sum the limbs over the ranks as
 *     int64.  A host that owns the reduction takes
 *       diag_limbs_len -> n = 6 nx_opd nv_opd + 6
 *       diag_local_exact -> limbs[n] of a species: [3 planes][2][nx_opd nv_opd] (hi row, lo row, as charge_local_exact:
 *         a bin's total is hi 2^32 + lo quanta) then [3 sums][2] (hi, lo),
 *     sums them element by element over the ranks (lo need not be normalised) and hands them to
 *       diag_convert_exact -> sums[3] as energy_sums and dist[3 nx_opd nv_opd + 3 nv_opd] as ptcldist(finish = 0)
 *         return them (either may be NULL); ptcldist_finish and output_scalars_from take over from there.
 *     diag_convert is the same conversion from the input alone (no context, no device).
 *   diag_quantise: n = rint(term 2^-log2_quantum) as the pass forms it (kinetic = 0: limit 2^44; 1: 2^62), or
 *     PIC1DP_ERR_ARG for a term the pass would not sum.  Host only. */
int pic1dp_hip_set_diag_sum(pic1dp_ctx *ctx, int32_t kind);
int pic1dp_hip_diag_quanta(const pic1dp_input *in, int32_t ispecies, int32_t log2_quantum[6]);
int pic1dp_hip_diag_quantise(double term, int32_t log2_quantum, int32_t kinetic, int64_t *n);
int pic1dp_hip_diag_limbs_len(pic1dp_ctx *ctx, int64_t *n);
int pic1dp_hip_diag_local_exact(pic1dp_ctx *ctx, int32_t ispecies, int64_t *limbs);
int pic1dp_hip_diag_convert_exact(pic1dp_ctx *ctx, int32_t ispecies, const int64_t *limbs, double sums[3], double *dist);
int pic1dp_hip_diag_convert(const pic1dp_input *in, int32_t ispecies, const int64_t *limbs, double sums[3], double *dist);

/* ---- state digest, checkpoint and restart (the file format: INTEGRATION.md 7) -----------------
 * THE DIGEST.  For species s and array k (0 x, 1 v, 2 w, 3 p of the current particle set) take every slot i in
 * [0, nalloc_s) -- the tail slots beyond np included; i is the logical index, as particles_download orders the
 * slots, not the offset in the tiled storage -- and let u be the 64 bits of the double:
 *     z = u + (i + 1) * 0x9E3779B97F4A7C15         (mod 2^64)
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     z =  z ^ (z >> 31)
 *     D[s][k] = sum over i of z                    (mod 2^64)
 * An integer sum: its order does not matter.  It depends on position (swapping two different markers changes it)
 * and on every bit (+0 and -0 differ, and so do NaN payloads).
 * state_digest: out[nspecies][4] = D of the markers on the device, in one streaming pass per species (32 B read
 *   per slot).  A noted push is put into memory first, exactly as pic1dp_hip_particles_download does; between time
 *   steps it launches the digest kernel only, waits, and changes nothing: the one-pass prediction and the cached
 *   diagnostics survive.
 * host_digest: the same sum over a host array of n doubles, *out = D (no device, no context). */
int pic1dp_hip_state_digest(pic1dp_ctx *ctx, uint64_t *out);
int pic1dp_hip_host_digest(const double *a, int64_t n, uint64_t *out);

/* ---- velocity moments of the markers on the field grid ------------------------
 * pic1dp_hip_moments(ctx, ispecies, which, out): the moments sum q v^k, k = 0 ... 3, of one species' markers, deposited
 * on the nx cells of the field grid with the deposit's own linear weights, computed on the device in streaming passes.
 *   - which is 1 (weights p: total f), 2 (weights w: delta f) or 3 (both, p first).
 *   - out[(j * 4 + k) * nx + ix], where j counts the selected weight sets in that order and k = 0 ... 3 is the power of v:
 *     4 nx doubles for which = 1 or 2, 8 nx for which = 3.
 *   - The sums are raw: no nx / lx, no Z, no background.
 * For every valid marker i < np of the species, on the state a pic1dp_hip_particles_download at that moment would return:
 *     px = wrap(x)                  the deposit's wrap (src/pic1dp_interaction.F90:102-104), NOT stored back
 *     (ix, wl) = locate(px)         the deposit's cell and left weight; ix == nx folds to 0; ir = (ix + 1 == nx) ? 0 : ix + 1
 *     a0 = wl * q                   q = p or w: the very products of the deposit
 *     b0 = (1.0 - wl) * q
 *     a1 = a0 * v    a2 = a1 * v    a3 = a2 * v        likewise b1 ... b3: every product rounded separately
 *     M[q][k][ix] += a_k            M[q][k][ir] += b_k
 *   - Tail slots (i >= np) do not count.
 *   - Markers with |v| >= v_max do count; this is not the rule of output_ptcldist's histograms.
 *   - The arithmetic is plain IEEE.  A non-finite term makes its bin non-finite; there is no counter and no trap.
 *   - The sums are FP64 and their order is free: the result is defined up to that order.  With n_b terms in a bin and B
 *     workgroups, |result - exact sum| <= (n_b + B) 2^-53 sum |terms| to first order.
 *   - Plane (w, 0) is the charge of the species before  * Z * nx / lx.  Normalisations, with f = total (p) or delta f (w):
 *     density n = M0 nx / lx, current J = Z M1 nx / lx, second moment (pressure + flow) P = m M2 nx / lx, third moment
 *     (heat flux + convected terms) Q = m M3 nx / lx; a full-f run (deltaf = 0) subtracts its background n0 itself.
 *   - which & 2 on a full-f context (deltaf = 0, no w) is PIC1DP_ERR_ARG; so are an unknown `which` and an unknown species.
 *   - The result is LOCAL to the context: the sum over ranks is an element-wise addition by the host, as with
 *     pic1dp_hip_charge_local.  No communicator is used.
 *   - pic1dp_hip_set_diag_sum and pic1dp_hip_set_charge_sum do not affect the call.  The exact (fixed-quanta) kind is an
 *     entry point of its own: pic1dp_hip_moments_exact below.
 * When the call may come.  Between time steps it launches its own passes and nothing else and changes nothing: markers,
 * fields, the one-pass prediction, a pending fused solve and cached diagnostics survive (the rule of
 * pic1dp_hip_state_digest).  Inside a time step (a push noted) it first puts the noted push into memory, as every entry point
 * outside the sequence does; the moments are those of the memory eager calls would hold.  Between charge_local and
 * charge_reduced (or their _exact pair), and with a half-step field waiting for the solve_field that adopts it, the call is
 * served as pic1dp_hip_particles_download is served there: from the markers as eager calls would hold them at that point (a
 * noted push becomes memory), and the charge_reduced or solve_field that follows does what it does after eager calls.  The
 * same holds for moments_exact / moments_local_exact, power and its exact kinds, select, select_count,
 * gather and state_digest; pic1dp_hip_output_all, which hands out field_chargeden, returns PIC1DP_ERR_STATE while a
 * charge_local is pending, as energy_sums, output_scalars and ptcldist do.  (tests/test_gpu_call_sequences.py calls every one
 * of them at every boundary of the reference's six calls and between charge_local and charge_reduced.)
 * Cost: one pass over x, v and p and / or w (24 or 32 B per marker) while the selected planes fit a workgroup's LDS (all
 * eight up to nx 2400); four planes per pass up to nx 4800 (which = 3: two passes), two per pass beyond (four, or two). */
int pic1dp_hip_moments(pic1dp_ctx *ctx, int32_t ispecies, int32_t which, double *out);

/* ---- exact, order-independent velocity moments ------------------------------------
 * The moments above with integer sums: fixed by the input and the markers alone, independent of launch shape, storage order
 * of the markers and split over ranks.  The exactness is in the entry point, not in a mode: set_diag_sum and set_charge_sum
 * do not affect these calls, and the checkpoint carries nothing of them.
 *   Terms.  The very terms of pic1dp_hip_moments: for every valid marker i < np the deposit's wrap and locate,
 *     a0 = wl * q, b0 = (1.0 - wl) * q, a_k = a_(k-1) * v, b_k alike, every product rounded on its own; a_k goes to cell ix,
 *     b_k to cell ir.  The chain runs through powers a pass does not hold, so a term has the same bits whichever pass adds
 *     it.  Tail slots do not count.
 *   Quanta.  Term t of plane (q, k) becomes n = rint(t 2^-e[k]), one rounding to nearest even, with
 *         e[k] = kb + k * kvm - 40          the same for q = p and q = w,
 *     kb = ceil(log2 B_s), B_s the bound of pic1dp_hip_charge_quantum (kb = charge_quantum + 52), kvm = ceil(log2 v_max).
 *     A term of 2^44 quanta or more, or a NaN, is not summed: it is counted per plane instead.  At the bounds |q| <= B_s
 *     and |v| <= v_max a term is at most 2^40 quanta, so the loader's markers are always in range, with a factor 16 of
 *     headroom for |q| |v|^k.
 *   Sums.  The integers are summed exactly -- in the LDS, across workgroups, across passes, and across ranks by the host.
 *     A bin's total is converted to double once (round to nearest even) and multiplied by 2^e[k].
 *   Limbs.  limbs[((j * 4 + k) * 2 + h) * nx + ix] as int64: j counts the selected weight sets in output order (p first),
 *     k is the power of v, h = 0 the hi limb, h = 1 the lo limb; a bin's total is hi 2^32 + lo quanta.  What
 *     moments_local_exact hands out is NORMALISED, 0 <= lo < 2^32: the limbs themselves are fixed by the markers.  What
 *     moments_convert accepts need not be: element-wise sums over ranks (MPI_Allreduce of MPI_INT64_T) are accepted.
 * moments_quanta: e[4] of a species from the input alone.  Host only.
 * moments_limbs_len: *n = 8 nx per selected weight set (which = 1, 2: 8 nx; 3: 16 nx).  Host only.
 * moments_local_exact: this context's exact sums as limbs.  Validation, the rule for a noted push and "between time steps
 *   nothing changes" are those of pic1dp_hip_moments.  No communicator is used.
 * moments_convert: limbs -> out, laid out as pic1dp_hip_moments lays it out.  Host only.
 * moments_exact: moments_local_exact followed by moments_convert, for one rank.
 *   - Terms that were not summed: the call returns PIC1DP_ERR_ARG naming the species, the weight set, the power and the
 *     count, and writes nothing to the caller's buffer.  The next call starts from zero counters: a counted error path, no
 *     trap.  Markers the call cannot sum are the caller's to fix; pic1dp_hip_moments is unaffected.
 *   - which & 2 on a full-f context or input, an unknown `which`, an unknown species and a null pointer are PIC1DP_ERR_ARG. */
int pic1dp_hip_moments_quanta(const pic1dp_input *in, int32_t ispecies, int32_t log2_quantum[4]);
int pic1dp_hip_moments_limbs_len(int32_t which, int32_t nx, int64_t *n);
int pic1dp_hip_moments_local_exact(pic1dp_ctx *ctx, int32_t ispecies, int32_t which, int64_t *limbs);
int pic1dp_hip_moments_convert(const pic1dp_input *in, int32_t ispecies, int32_t which, const int64_t *limbs, double *out);
int pic1dp_hip_moments_exact(pic1dp_ctx *ctx, int32_t ispecies, int32_t which, double *out);

/* ---- velocity-resolved wave-particle power on the output grid ---------------------
 * pic1dp_hip_power(ctx, ispecies, which, out): the power the field does on the markers, q v E(x) per marker, of one species,
 * resolved on the nx_opd x nv_opd output grid of output_ptcldist (the field-particle correlation), computed on the device in
 * streaming passes over the markers with the field in the workgroups' LDS.
 *   - which is 1 (weights p: total f), 2 (weights w: delta f) or 3 (both, p first).
 *   - out, per selected weight set in that order: [nv_opd * nx_opd plane | nv_opd v-profile | rest], that is
 *     nx_opd * nv_opd + nv_opd + 1 doubles per set; the plane's index is iv * nx_opd + ix.
 *   - pic1dp_hip_power_len(in, which, &n): n = nsets * (nx_opd * nv_opd + nv_opd + 1).  Host only.
 * For every valid marker i < np of the species, on the state a pic1dp_hip_particles_download at that moment would return,
 * with E = field_electric as pic1dp_hip_get_field would return it at that moment:
 *     px = wrap(x)                                  the deposit's wrap (src/pic1dp_interaction.F90:102-104), NOT stored back
 *     (ix, wl) = locate(px)                         ix == nx folds to 0; ir = (ix + 1 == nx) ? 0 : ix + 1
 *     e = E[ix] * wl;  e = e + E[ir] * (1.0 - wl)   the push's gather, in the push's order (src/pic1dp_interaction.F90:254-257)
 *     c = v * e
 *     t_q = c * q                                   q = p and / or w
 *   - Bins.  The four cells and bilinear weights of output_ptcldist's histograms (src/pic1dp_output.F90:239-315) for
 *     (px, v), edge rules included: the x cell nx_opd folds to 0, the right-hand neighbour of the last x cell is cell 0, the
 *     top v row keeps a marker whose upper row would carry weight 0, and |v| >= v_max gives no bins.
 *         P[q][c00] += w00 * t_q    P[q][c01] += w01 * t_q    P[q][c10] += w10 * t_q    P[q][c11] += w11 * t_q
 *     with w00 = sx * sv, w01 = sx * svu, w10 = sxr * sv, w11 = sxr * svu as the histograms form them.
 *   - A marker without bins adds t_q to one scalar per set: rest[q] += t_q.  Bins plus rest account for every marker.
 *   - The v-profile is the plane summed over ix ascending, in doubles, on the host after the transfer.
 *   - Tail slots (i >= np) do not count.
 *   - The arithmetic is plain IEEE, every product and sum rounded on its own.  A non-finite term makes its bin non-finite;
 *     there is no counter and no trap.
 *   - The sums are FP64 and their order is free: the result is defined up to that order.  With n_b terms in a bin (or in
 *     rest) and B workgroups, |result - exact sum| <= (n_b + B) 2^-53 sum |terms| to first order.  The exact
 *     (integer) kind of these planes is an entry point of its own: pic1dp_hip_power_exact below.
 *   - Normalisation.  The sums are raw and LOCAL to the context: the sum over ranks is an element-wise addition by the
 *     host; no communicator is used.  Z_s * t is the rate at which the field does work on that marker's share of f (q = p)
 *     or delta f (q = w); 2 (Z / m) sum t_w is the part of d/dt sum v^2 w that comes from the acceleration at fixed weights.
 *     No nx / lx, no bin widths: divide by (lx / nx_opd) (2 v_max / (nv_opd - 1)) for a density in (x, v).
 *   - which & 2 on a full-f context (deltaf = 0, no w) is PIC1DP_ERR_ARG; so are an unknown `which`, an unknown species, a
 *     null pointer, and nx_opd < 1 or nv_opd < 2.
 *   - pic1dp_hip_set_diag_sum and pic1dp_hip_set_charge_sum do not affect the call, and the checkpoint carries nothing of it.
 * When the call may come.  The rule of pic1dp_hip_moments, and pic1dp_hip_get_field's for the field.  Between time steps it
 * launches its own passes and nothing else and changes nothing: markers, fields, the one-pass prediction, the fused solve
 * and cached diagnostics survive.  Inside a time step (a push noted) the noted push becomes memory first; markers and field
 * are then those eager call sites would hold.  Between charge_local and charge_reduced: as pic1dp_hip_moments, with the
 * field pic1dp_hip_get_field shows there.
 * Cost: one pass over x, v and p and / or w (24 or 32 B per marker) while the E tile (8 (nx + 1) B) and the selected planes
 * fit a workgroup's LDS (150 KiB); one pass per set where only one plane fits; planes that do not fit at all are summed
 * straight in memory. */
int pic1dp_hip_power(pic1dp_ctx *ctx, int32_t ispecies, int32_t which, double *out);
int pic1dp_hip_power_len(const pic1dp_input *in, int32_t which, int64_t *n);   /* host only */

/* ---- exact, order-independent wave-particle power ---------------------------------
 * The planes above with integer sums: fixed by the input, the markers and the field alone, independent of launch shape,
 * storage order of the markers, number of passes and split over ranks.  The exactness is in the entry points, not in a mode:
 * set_diag_sum and set_charge_sum do not affect these calls, and the checkpoint carries nothing of them.
 *   Terms.  The very terms of pic1dp_hip_power, bit for bit: px = wrap(x), (ix, wl) = locate(px), e = E[ix] * wl;
 *     e = e + E[ir] * (1.0 - wl), c = v * e, t_q = c * q.  A marker with bins contributes the four products w00 * t_q ...
 *     w11 * t_q of the output grid's stencil with its edge rules; a marker with |v| >= v_max contributes t_q to rest[q].
 *     Tail slots do not count.
 *   Scale.  A term t becomes n = rint(t 2^-e), one rounding to nearest even, with
 *         e = max(kb + kvm + kE - 40, -1000)        one e for p and w, the planes and rest,
 *     kb = ceil(log2 B_s), B_s the bound of pic1dp_hip_charge_quantum (kb = charge_quantum + 52), kvm = ceil(log2 v_max),
 *     kE = ceil(log2 max_ix |E[ix]|) over the field pic1dp_hip_get_field would return at that moment, kE = 0 for a field of
 *     zeros (all terms are then +-0 and all limbs 0).  The clamp keeps 2^e and 2^-e normal doubles for a subnormal field.
 *     The quantum follows the field of the call: max |E| is found on the device, and e is handed out with the limbs.
 *     At the bounds |q| <= B_s, |v| <= v_max, |e| <= max |E| a binned term is at most 2^40 (1 + a few ulp) quanta.  A term of
 *     2^44 quanta or more, or a NaN, is not summed: it is counted, per weight set, separately for bins and for rest.
 *     A field with an infinity or a NaN is PIC1DP_ERR_ARG ("field not finite"); no marker is read.
 *   Sums.  The integers are summed exactly -- in the LDS, across workgroups, across passes, and across ranks by the host.
 *     Each bin's total, and each rest total, is converted to double once (round to nearest even) and multiplied by 2^e.  The
 *     v-profile is the exact integer sum over ix of the plane's bins, converted once -- not the sum of the converted doubles.
 *   Limbs.  Per selected weight set j, in output order (p first), power_limbs_len / nsets int64 words:
 *         [hi plane: nv_opd * nx_opd | lo plane: nv_opd * nx_opd | rest hi | rest lo]
 *     a total is hi 2^32 + lo quanta, the plane's index is iv * nx_opd + ix.  What power_local_exact hands out is NORMALISED,
 *     0 <= lo < 2^32: the limbs are fixed by the markers and the field.  What power_convert accepts need not be:
 *     element-wise sums over ranks (MPI_Allreduce of MPI_INT64_T) are accepted as they are.
 *   Ranks.  The field is bit-identical on all ranks, so e is too: the host checks that the ranks' e agree, adds the limbs
 *     and converts once.
 * power_quantum: e of a species from the input and max |E| -- the rule above.  max_abs_E negative, infinite or NaN:
 *   PIC1DP_ERR_ARG.  Host only.
 * power_limbs_len: *n = nsets * (2 * nx_opd * nv_opd + 2).  Host only.
 * power_local_exact: this context's exact sums as limbs, and the call's e.  Validation, the rule for a noted push and
 *   "between time steps nothing changes" are those of pic1dp_hip_power.  No communicator is used.
 * power_convert: limbs and e -> out, laid out as pic1dp_hip_power lays it out.  Host only.
 * power_exact: power_local_exact followed by power_convert, for one rank.
 *   - Terms that were not summed: the call returns PIC1DP_ERR_ARG naming the species, the weight set, bins or rest and the
 *     count, and writes nothing to the caller's buffers.  The next call starts from zero counters: a counted error path, no
 *     trap.  Markers the call cannot sum are the caller's to fix; pic1dp_hip_power is unaffected.
 *   - which & 2 on a full-f context or input, an unknown `which`, an unknown species, a null pointer, and nx_opd < 1 or
 *     nv_opd < 2 are PIC1DP_ERR_ARG.
 * Cost: pic1dp_hip_power's passes (the planes are 64-bit words, byte for byte the doubles' size), on the grid of the exact
 * kinds: one workgroup per 2^17 markers, at most one per CU. */
int pic1dp_hip_power_quantum(const pic1dp_input *in, int32_t ispecies, double max_abs_E, int32_t *log2_quantum);   /* host only */
int pic1dp_hip_power_limbs_len(const pic1dp_input *in, int32_t which, int64_t *n);                                 /* host only */
int pic1dp_hip_power_local_exact(pic1dp_ctx *ctx, int32_t ispecies, int32_t which, int64_t *limbs, int32_t *log2_quantum);
int pic1dp_hip_power_convert(const pic1dp_input *in, int32_t which, int32_t log2_quantum, const int64_t *limbs, double *out);   /* host only */
int pic1dp_hip_power_exact(pic1dp_ctx *ctx, int32_t ispecies, int32_t which, double *out);

/* ---- select and gather markers on the device: phase-space samples and tracers ----------
 * pic1dp_hip_select hands out the markers of one species that lie in a window of (x, v), thinned by a hash of their global
 * index, in ascending logical index; pic1dp_hip_gather hands out the markers at given logical indices.  Neither moves the
 * species over PCIe: what crosses is 40 B (select) or 32 B (gather) per marker handed out. */
typedef struct pic1dp_select {
  double x_lo, x_hi;   /* window in the WRAPPED position px */
  double v_lo, v_hi;   /* window in v */
  uint64_t thin;       /* 0: keep every marker of the window; else keep iff h(g) < thin */
  uint64_t key;        /* of the thinning hash */
  int64_t origin;      /* g = origin + i: pass pic1dp_hip_load_origin's G0 and a sample no longer depends on the split over ranks */
} pic1dp_select;
/* The rule.  It applies to every valid marker i < np of the species, in the logical order of pic1dp_hip_particles_download,
 * on the state a pic1dp_hip_particles_download at that moment would return:
 *     px = wrap(x)                                  the deposit's wrap (src/pic1dp_interaction.F90:102-104: fmod, then + lx
 *                                                   where negative), NOT stored back; px == lx, the known rounding case of
 *                                                   a tiny negative x, is used as it is
 *     in_x = x_lo <= px && px < x_hi                when x_lo <= x_hi
 *     in_x = px >= x_lo || px < x_hi                when x_lo > x_hi: the window straddles the periodic boundary
 *     in_v = v_lo <= v && v < v_hi
 *     h(g) = mix64(key + (g + 1) * 0x9E3779B97F4A7C15) mod 2^64,  g = origin + i      (mix64: particle_load_device above)
 *     selected = in_x && in_v && (thin == 0 || h(g) < thin)
 *   - Bounds.  +-inf bounds are allowed: that is how a caller says "all".  x_lo == x_hi is the empty window.
 *     A NaN bound is PIC1DP_ERR_ARG.  A NaN px or v is never selected: every comparison with it is false.  The upper
 *     bounds are strict, so neither is v = +inf (an infinite x wraps to NaN).
 *   - Thinning.  The hash depends on the marker's index alone, not on its values: the same markers are kept at every
 *     time, which makes a thinned selection a tracer set.  It is a hash and not a stride: global marker g of a quiet
 *     start has u_v = bitrev64(g) 2^-64, so "every 2^k-th marker" is one band of velocities.
 *     pic1dp_hip_select_thin(fraction, &thin): fraction >= 1 gives 0 (keep all), fraction <= 0 or NaN is PIC1DP_ERR_ARG,
 *     otherwise thin = max(1, floor(fraction 2^64)).  Host only.
 *   - Tail slots (i >= np) are never selected, whatever they hold.
 *   - Output.  The selected markers in ascending i: the stored bits of x (unwrapped, as download gives it), v, p and w,
 *     and i itself.  On a full-f context (deltaf = 0) w is whatever pic1dp_hip_particles_download gives there.  The
 *     result equals a boolean mask on the downloaded arrays bit for bit, whatever the launch shape.
 * pic1dp_hip_select_count: *count = the number of markers selected.
 * pic1dp_hip_select: *count = the number selected (the total, whatever max is); the first min(count, max) of them are
 *   written to index, x, v, p, w (max elements each), so truncation shows as count > max.  Any output pointer may be NULL
 *   (that array is not handed out).  max = 0 is legal and equals select_count.  max < 0, a null sel or count, a NaN bound
 *   or an unknown species is PIC1DP_ERR_ARG with nothing written.
 * pic1dp_hip_gather: x[k], v[k], p[k], w[k] (any may be NULL) = the values of the marker at logical index index[k],
 *   k < n.  Indices in any order, duplicates allowed, 0 <= index < nalloc: tail slots included, as download returns
 *   them.  The indices are checked on the host before anything is launched; one outside the range is PIC1DP_ERR_ARG
 *   naming the first offender.  n = 0 is a no-op that returns 0; n < 0 or a null index is PIC1DP_ERR_ARG.
 * pic1dp_hip_host_select: the rule on HOST arrays x, v of np markers (lx from the input): *count and the first
 *   min(count, max) logical indices (index may be NULL).  Host only, no device, no context.
 * When the calls may come.  The rule of pic1dp_hip_moments.  Between time steps they launch their own passes and nothing
 * else and change nothing: markers, fields, the one-pass prediction, a pending fused solve, cached diagnostics and the
 * state digest survive.  Inside a time step (a push noted) the noted push becomes memory first.  No communicator is used;
 * the results are LOCAL to the context.  pic1dp_hip_set_diag_sum and pic1dp_hip_set_charge_sum do not affect them, and
 * the checkpoint carries nothing of them.
 * Memory.  The chunk counts (8 B per 16384 markers), the device buffer of the result (min(count, max) x 40 B) and a
 * gather's index and result buffers (n x 40 B) live for the call only: the context's standing allocation does not grow.
 * An allocation that fails is PIC1DP_ERR_NOMEM.  The transfer to the host goes through the context's pinned staging in
 * slices of at most 32 MiB, as the checkpoint's does.
 * Cost: pic1dp_hip_select_count is one pass over x and v (16 B per marker) and a one-workgroup prefix sum of the chunk
 * counts; pic1dp_hip_select adds a second pass over x and v of the chunks that hold a selected marker of rank < max
 * (chunks without one are skipped), 16 B read of p and w and 40 B written per marker handed out.  No per-marker bitmap
 * is kept between the passes.  pic1dp_hip_gather is four 8-byte reads at random places and four stores per entry.
 * Measured at 1e8 markers on one MI355X, device time: select_count 0.26 ms (0.97 of a pure read stream
 * of x and v), a select of 2^20 markers 0.67 ms, a gather of 2^20 random indices 0.11 ms; 7 ms of wall clock per select
 * call with its transfer, against 600 ms for pic1dp_hip_particles_download and a mask on the host. */
int pic1dp_hip_select_count(pic1dp_ctx *ctx, int32_t ispecies, const pic1dp_select *sel, int64_t *count);
int pic1dp_hip_select(pic1dp_ctx *ctx, int32_t ispecies, const pic1dp_select *sel, int64_t max, int64_t *count,
                      int64_t *index, double *x, double *v, double *p, double *w);
int pic1dp_hip_gather(pic1dp_ctx *ctx, int32_t ispecies, const int64_t *index, int64_t n,
                      double *x, double *v, double *p, double *w);
int pic1dp_hip_host_select(const pic1dp_input *in, const pic1dp_select *sel, const double *x, const double *v, int64_t np,
                           int64_t max, int64_t *count, int64_t *index);          /* host only, no device */
int pic1dp_hip_select_thin(double fraction, uint64_t *thin);                      /* host only */

/* ---- exact phase-space histogram on a caller-chosen window and grid ----------------------
 * pic1dp_hip_zoom counts the markers of one species, and sums their p and w, on a cell-centred grid of nxb x nvb cells laid
 * over a window of (wrapped x, v) the caller chooses -- the picture pic1dp_hip_ptcldist draws on the input's fixed grid,
 * zoomed to where the physics is.  There is one kind only: exact.  A term is the marker's own p or w (no interpolation
 * weight), rounded once to whole quanta and summed as integers, so the result does not depend on launch shape, marker order,
 * the number of passes or the split over ranks. */
typedef struct pic1dp_zoom {
  double x_lo, x_hi;     /* window in the WRAPPED position px; x_lo > x_hi straddles the periodic boundary */
  double v_lo, v_hi;     /* window in v, v_lo < v_hi */
  int32_t nxb, nvb;      /* cells across the window */
} pic1dp_zoom;
/* which is a mask: 1 markr (the count of markers), 2 total (sum p), 4 pertb (sum w); the selected planes come in that order.
 * The rule.  It applies to every valid marker i < np of the species, on the state a pic1dp_hip_particles_download at that
 * moment would return.  Every operation is one IEEE operation; none of them has the shape of an FMA.
 *     px   = wrap(x)                                   the deposit's wrap, exactly as pic1dp_hip_select uses it; not stored back
 *     in_x = x_lo <= px && px < x_hi                   when x_lo <= x_hi
 *     in_x = px >= x_lo || px < x_hi                   when x_lo >  x_hi
 *     in_v = v_lo <= v && v < v_hi
 *     Lw   = x_hi - x_lo            (x_lo <= x_hi)     Lw = (x_hi + lx) - x_lo    (x_lo > x_hi)          host, once
 *     sx   = (double)nxb / Lw       sv = (double)nvb / (v_hi - v_lo)                                     host, once
 *     d    = px - x_lo;  if (d < 0) d = d + lx
 *     ix   = (int)(d * sx);         if (ix > nxb - 1) ix = nxb - 1
 *     jv   = (int)((v - v_lo) * sv); if (jv > nvb - 1) jv = nvb - 1
 *     cell = jv * nxb + ix
 *   - A marker with in_x && in_v adds terms to its cell: 1 to markr, p to total, w to pertb.  A marker outside the window
 *     adds nothing.  A NaN px or v is never inside the window.  Tail slots (i >= np) do not count.
 *   - The clamp is reachable at the upper edge of either axis (the product may round up to nxb or nvb just below the bound);
 *     the overshoot is one cell.  An inside marker never gives a negative index: d and v - v_lo are not negative.
 * Argument checks (PIC1DP_ERR_ARG, nothing written): the bounds finite, 0 <= x_lo, x_hi <= lx, v_lo < v_hi (stricter than
 *   pic1dp_hip_select: a grid needs a finite extent); v_hi - v_lo, sx and sv finite (so the window x_lo = lx, x_hi = 0, whose
 *   extent is zero although px == lx would lie in it, is refused); 1 <= nxb, nvb <= 4096 and
 *   nxb * nvb <= 2^20; which in 1..7; which & 4 on a full-f context or input (deltaf = 0); an unknown species; a null
 *   pointer.  x_lo == x_hi is legal and is the empty window: all zeros, and no marker is read.
 * Sums.  markr is a plain integer count: its quantum is one.  A term t of total or pertb becomes n = rint(t 2^-e), e =
 *   pic1dp_hip_diag_quanta's entry 1 (total) or 2 (pertb) of the species, kb - 40, from the input alone -- what
 *   pic1dp_hip_diag_quantise(t, e, 0, &n) hands out.  A term of 2^44 quanta or more, or a NaN, is not summed but counted,
 *   per plane: the call returns PIC1DP_ERR_ARG naming the species, the plane and the count, nothing is written to the
 *   caller's buffer, and the next call starts from zero counters.  Each plane judges its own term: a marker whose p is
 *   rejected still counts in markr.  The integers are summed exactly -- in a workgroup's LDS, across workgroups, across
 *   passes, and by the host across ranks.
 * Limbs: limbs[((j * 2 + h) * nvb + jv) * nxb + ix], j counting the selected planes, h = 0 the hi limb, h = 1 the lo limb;
 *   a cell's total is hi * 2^32 + lo quanta.  pic1dp_hip_zoom_local_exact hands out normalised limbs (0 <= lo < 2^32), so
 *   the limbs are fixed by the markers; pic1dp_hip_zoom_convert accepts element-wise sums over ranks as they are.
 *   out[(j * nvb + jv) * nxb + ix] is the total converted to double once (round to nearest even) times 2^e.  The sums are
 *   raw and local to the context: no communicator is used, and there are no bin widths -- dividing by
 *   (Lw / nxb) * ((v_hi - v_lo) / nvb) gives a density, which is the caller's line, as with pic1dp_hip_power.
 * pic1dp_hip_zoom_len / _zoom_limbs_len: nplanes * nxb * nvb doubles of out / twice as many limbs.  Host only.
 * pic1dp_hip_host_zoom: the rule and the sums on HOST arrays of np valid markers (p read where which & 2, w where which & 4):
 *   the normalised limbs of the terms summed, and rejected[3], the terms not summed per plane markr, total, pertb (it
 *   returns 0 with them counted: the caller sees both).  Host only, no device, no context.
 * pic1dp_hip_zoom_stats: the passes that swept markers so far, their device milliseconds while kernel stats were enabled,
 *   and the terms not summed so far (pic1dp_hip_kernel_stats keeps its rows 0..22).
 * When the call may come.  The rule of pic1dp_hip_moments.  Between time steps it launches its own passes and nothing else
 *   and changes nothing: markers, fields, the one-pass prediction, a pending fused solve, cached diagnostics and the state
 *   digest survive.  Inside a time step (a push noted) the noted push becomes memory first.  pic1dp_hip_set_diag_sum and
 *   pic1dp_hip_set_charge_sum do not affect it, and the checkpoint carries nothing of it.
 * Memory.  The device rows (16 B per plane and cell: up to 6 x 8 MiB) and the three counters live for the call only, as
 *   pic1dp_hip_select's buffers do: the context's standing allocation does not grow.  An allocation that fails is
 *   PIC1DP_ERR_NOMEM.  The transfer to the host goes through the context's pinned staging in slices of at most 32 MiB.
 * Cost.  Planes of up to 19 200 words (150 KiB of a workgroup's LDS; 64 x 64 x 3 fits) take one pass over x, v and the
 *   weights asked for.  A larger grid is cut into bands of whole v rows, one pass each, whose per-marker test begins with
 *   v: a pass over a band the marker is not in costs its loads, two compares and a product.  Beyond the plan's pass cap
 *    one pass adds every term straight into the global rows with two 64-bit atomics. */
int pic1dp_hip_zoom_len(const pic1dp_zoom *z, int32_t which, int64_t *n);        /* host only: nplanes * nxb * nvb     */
int pic1dp_hip_zoom_limbs_len(const pic1dp_zoom *z, int32_t which, int64_t *n);  /* host only: 2 * nplanes * nxb * nvb */
int pic1dp_hip_zoom_local_exact(pic1dp_ctx *ctx, int32_t ispecies, const pic1dp_zoom *z, int32_t which, int64_t *limbs);
int pic1dp_hip_zoom_convert(const pic1dp_input *in, int32_t ispecies, const pic1dp_zoom *z, int32_t which,
                            const int64_t *limbs, double *out);                  /* host only */
int pic1dp_hip_zoom(pic1dp_ctx *ctx, int32_t ispecies, const pic1dp_zoom *z, int32_t which, double *out);
int pic1dp_hip_host_zoom(const pic1dp_input *in, int32_t ispecies, const pic1dp_zoom *z, int32_t which, const double *x,
                         const double *v, const double *p, const double *w, int64_t np, int64_t *limbs,
                         int64_t rejected[3]);                                   /* host only: the rule on HOST arrays */
int pic1dp_hip_zoom_stats(pic1dp_ctx *ctx, double *ms, int64_t *passes, int64_t *rejected);

/* ---- Fourier-Hermite spectrum of f and delta f, summed on the matrix unit ----------------
 * pic1dp_hip_hermite(ctx, ispecies, which, h, out): the Hermite spectrum of the Fourier modes of one species' markers,
 * g_{k,n} = sum_i q_i psi_n(u_i) exp(-i k x_i) -- the measure of phase mixing (Landau damping, bump-on-tail): |g_{k,n}|^2
 * against n is the free-energy spectrum of mode k, its front moves as n ~ (k v_t t)^2, its floor is the marker noise.
 * Evaluated per marker it is unbiased and needs no velocity grid.  It is a matrix product over the marker index,
 * G[n][c] = sum_i Psi[n][i] Y[i][c], and is summed by the FP64 matrix unit (v_mfma_f64_16x16x4_f64). */
typedef struct pic1dp_hermite {
  int32_t nherm, nmodes;   /* Hermite rows n = 0 .. nherm - 1; Fourier modes listed in modes[0 .. nmodes) */
  int32_t modes[8];
  double v0, vt;           /* u = (v - v0) / vt */
} pic1dp_hermite;
/*   - which is 1 (weights p: total f), 2 (weights w: delta f) or 3 (both, p first).
 *   - 1 <= nherm <= 256; 1 <= nmodes and nsets * nmodes <= 8 (sixteen columns); the modes distinct, 0 <= m <= nx / 2; vt
 *     finite and > 0, v0 finite.  Anything else is PIC1DP_ERR_ARG, and so are which & 2 on a full-f context (deltaf = 0), an
 *     unknown species and a null pointer; nothing is written then.
 *   - out[((j * nmodes + a) * 2 + t) * nherm + n], j the selected weight set, a the index into modes, t = 0 the cos sum C,
 *     1 the sin sum S.  pic1dp_hip_hermite_len(h, which, &n): n = nsets * nmodes * 2 * nherm.  Host only (the modes are
 *     not held against nx there).
 * For every valid marker i < np of the species, on the state a pic1dp_hip_particles_download at that moment would return:
 *     px = wrap(x)                                   the deposit's wrap (src/pic1dp_interaction.F90:102-104), NOT stored back
 *     u  = (v - v0) * ivt                            ivt = 1.0 / vt, computed once on the host
 *     psi_0 = 1;  psi_1 = u;  psi_(n+1) = (u * psi_n) * ra[n] - psi_(n-1) * rb[n]
 *         ra[n] = 1.0 / sqrt((double)(n + 1)),  rb[n] = sqrt((double)n) / sqrt((double)(n + 1)), IEEE sqrt and division
 *         (pic1dp_hip_hermite_tables hands them out); every product and the difference rounded on their own.  These are the
 *         orthonormal probabilists' Hermite polynomials: the integral of psi_m psi_n exp(-u^2 / 2) / sqrt(2 pi) is delta_mn.
 *     theta = kk[a] * px                             kk[a] = 2.0 * pi / lx * (double)modes[a], the loader's expression
 *     (s, c) = sincos(theta)                         the device library's
 *     y_cos = q * c;  y_sin = q * s                  q = p and / or w
 *     out[j][a][0][n] += psi_n * y_cos;  out[j][a][1][n] += psi_n * y_sin
 *   - g_{k,n} = C - i S is the coefficient of exp(+i k x) psi_n(u) exp(-u^2 / 2) / sqrt(2 pi) in the species' f (q = p) or
 *     delta f (q = w).  For mode 0 the sin row is exactly 0.
 *   - Tail slots (i >= np) do not count, whatever they hold (a NaN included).
 *   - The sums are FP64; their order, and whether a product is fused into its addition, are free.  With n_p valid markers, T
 *     the float64 terms psi_n * y and B the partial sums the launch merges (pic1dp_probe_host_hermite_plan says how many):
 *     |out - exact sum T| <= (n_p + B + 16) 2^-53 sum |T| (1 + 2^-20); the 16 covers sincos within 4 ulp and the two products.
 *     A non-finite marker makes sums non-finite; there is no counter and no trap.
 *   - Normalisation.  The sums are raw and LOCAL to the context: the sum over ranks is an element-wise addition by the host.
 *   - pic1dp_hip_set_diag_sum and pic1dp_hip_set_charge_sum do not affect the call, and the checkpoint carries nothing of it.
 * When the call may come.  The rule of pic1dp_hip_moments.  Between time steps it launches its own pass and nothing else and
 * changes nothing; inside a time step (a push noted) the noted push becomes memory first.
 * Memory.  4 KiB of tables and 32 KiB of sums on the device, allocated at the first call and kept by the context.
 * Cost: one pass over x, v and p and / or w (24 or 32 B per marker), nmodes sincos per marker, and one matrix instruction
 * per marker and 64 Hermite rows (nherm is rounded up to 64, 128 or 256 rows of work).
 * pic1dp_hip_host_hermite: the same terms on HOST arrays of np valid markers (p read where which & 1, w where which & 2), with
 *   the host library's sincos, summed in marker order in doubles.  Host only, no device, no context.
 * pic1dp_hip_hermite_stats: the passes launched so far and their device milliseconds while kernel stats were enabled
 *   (pic1dp_hip_kernel_stats keeps its rows 0..22). */
int pic1dp_hip_hermite_len(const pic1dp_hermite *h, int32_t which, int64_t *n);      /* host only */
int pic1dp_hip_hermite(pic1dp_ctx *ctx, int32_t ispecies, int32_t which, const pic1dp_hermite *h, double *out);
int pic1dp_hip_host_hermite(const pic1dp_input *in, int32_t ispecies, int32_t which, const pic1dp_hermite *h,
                            int64_t np, const double *x, const double *v, const double *p, const double *w, double *out);  /* host only */
int pic1dp_hip_hermite_tables(int32_t nherm, double *ra, double *rb);                /* host only */
int pic1dp_hip_hermite_stats(pic1dp_ctx *ctx, double *ms, int64_t *passes);

/* what pic1dp_hip_checkpoint_info reports of a file besides the input */
typedef struct pic1dp_checkpoint_info {
  int32_t format_version;
  int32_t nspecies;
  int64_t file_bytes;
  int64_t input_size;          /* sizeof(pic1dp_input) of the writer */
  pic1dp_layout layout;        /* rank, nranks, npe of the writing context; device = -1 */
  int32_t settings[8];         /* charge_sum, diag_sum, field_transform, field_solver, step_mode, output fusion,
                                  seed_offset; one spare */
  int32_t itime, nblk;         /* global_itime; reference blocks the writer owned */
  double time;
  int32_t imerge, iremove, isplit, rng_ready;  /* the events' counters; 1: the file carries the blocks' generators */
  int64_t hist_count;          /* entries of the energy history */
  int64_t nalloc[PIC1DP_MAX_SPECIES], np[PIC1DP_MAX_SPECIES];
  uint64_t digest[PIC1DP_MAX_SPECIES][4];      /* D[s][k] of the marker sections */
  uint64_t checksum;           /* of everything else */
} pic1dp_checkpoint_info;

/* checkpoint_write: everything that decides later bits into ONE file per context (per rank; no collective call):
 *   input, layout and the seven settings above; itime and time; per species nalloc, np, the per-block counts and
 *   x, v, w, p in logical order (untiled); field_electric, field_chargeden, the kept modes; the energy history; the
 *   events' counters and every owned block's generator; the prediction tiles' fixed-point bounds; the diagnostics
 *   pass's scales; the digests of the marker sections and one checksum over the rest.
 *   Only between time steps: inside one, or with a charge_local pending, it returns PIC1DP_ERR_STATE and creates no
 *   file; the context goes on as if the call had not come.  "Inside a time step" is decided by the calls alone, the same
 *   with lazy and with eager call sites: push(1) and push(2) open their sub-step, the collect_charge (or charge_reduced)
 *   and the solve_field that follow move on, and the time step is over behind the solve_field of the second sub-step --
 *   so the write is refused after each of the first five of the reference's six calls push(1), collect_charge,
 *   solve_field, push(2), collect_charge, solve_field (the file carries no RK backup for a push(2), and behind the second
 *   collect_charge the field of the new state is still to be solved).  substep(1) leaves the context inside a time
 *   step; substep(2), step, a particle load, an upload and checkpoint_read leave it between two.
 *   What collect_charge left to the next solve_field is settled first.  The markers cross in chunks through
 *   the context's pinned staging; the file appears under its name only when it is complete.
 *   Afterwards everything the file does NOT carry -- the one-pass prediction, the predicted half-step field, cached
 *   diagnostics, the accumulator sets, the call sites' state -- is put into the one defined state that
 *   checkpoint_read produces too: THE WRITING CONTEXT AND A CONTEXT RESTORED FROM THE FILE CONTINUE BIT FOR BIT
 *   ALIKE.  The price: the step after a checkpoint takes two passes over the markers.
 * checkpoint_read: into a context created with the same input and layout and set to the same seven settings --
 *   otherwise PIC1DP_ERR_ARG naming the first field that differs, the context untouched.  Lengths and checksum are
 *   verified before the device is touched; then the markers are uploaded, the digest kernel runs and its words are
 *   compared with the file's: a mismatch returns PIC1DP_ERR_ARG naming species and array and leaves the context
 *   without markers (the next step reports "no particles").  Touches neither communicator nor exchange.
 * checkpoint_info: input (may be NULL) and the description above, from a file whose lengths and checksum hold.
 * checkpoint_verify: info's checks and every marker section against its digest (pic1dp_hip_host_digest), naming
 *   what fails.  Both host only: no device, no context. */
int pic1dp_hip_checkpoint_write(pic1dp_ctx *ctx, const char *path);
int pic1dp_hip_checkpoint_read(pic1dp_ctx *ctx, const char *path);
int pic1dp_hip_checkpoint_info(const char *path, pic1dp_input *in, pic1dp_checkpoint_info *info);
int pic1dp_hip_checkpoint_verify(const char *path);

/* ---- multi-GPU: RCCL communicator (replaces MPI_Allreduce at
 * src/pic1dp_interaction.F90:132) ------------------------------------------
 * rank 0 obtains an id, the host distributes the 128 bytes to every rank
 * (MPI_Bcast / torch.distributed), every rank calls comm_init.  A context with
 * nranks = 1 needs no communicator; if comm_init is called on it anyway a
 * 1-rank communicator is created and the all-reduce path is taken (used to
 * exercise that path on a single GPU). */
int pic1dp_hip_comm_unique_id(unsigned char id[PIC1DP_COMM_ID_BYTES]);
int pic1dp_hip_comm_init(pic1dp_ctx *ctx,
                         const unsigned char id[PIC1DP_COMM_ID_BYTES]);

/* 0 when librccl can be loaded in this process (no device touched): lets every
 * rank of a job agree on RCCL before any of them enters ncclCommInitRank */
int pic1dp_hip_comm_available(void);

/* ---- multi-GPU alternative: one-hop charge exchange (also replaces MPI_Allreduce
 * at src/pic1dp_interaction.F90:132) ------------------------------
 * Every rank keeps one slot per source rank; after its deposit a rank stores its
 * charge vector into its slot on every GPU of the node (peer-mapped memory, one
 * xGMI hop), then every GPU adds the slots in rank order inside the field
 * solve's launch: one launch per sub-step instead of three, and the summed charge
 * -- hence E and the trajectories -- are bit-identical on all ranks and from run to
 * run.  Set-up: every rank calls xchg_create and hands its 64-byte handle to all
 * ranks (MPI_Allgather / torch.distributed.all_gather); every rank then calls
 * xchg_connect with the nranks handles in rank order (handles[rank] is its own),
 * and set_allreduce(2) on all ranks at the same point of the run.  Ranks may be
 * separate processes (the areas are mapped through hipIpc) or contexts of ONE
 * process, each driven by its own host thread (a handle made in this process is
 * recognised and its area addressed directly, with peer access enabled when it
 * lies on another device): the reference's `mpiexec -n N` either way.  A rank that
 * waits longer than PIC1DP_XCHG_TIMEOUT_MS (default 20 000) for a peer gives up:
 * the kernels always finish and the next synchronising call returns
 * PIC1DP_ERR_COMM. */
int pic1dp_hip_xchg_create(pic1dp_ctx *ctx, unsigned char handle[PIC1DP_XCHG_HANDLE_BYTES]);
int pic1dp_hip_xchg_connect(pic1dp_ctx *ctx, const unsigned char *handles);
/* which reduction collect_charge / substep / step use from now on:
 * 0 auto (RCCL when a communicator exists), 1 RCCL, 2 the one-hop exchange */
int pic1dp_hip_set_allreduce(pic1dp_ctx *ctx, int32_t kind);
/* memory kind of the exchange area (1 fine-grained, 2 uncached, 3 plain device
 * memory), exchanges performed so far; returns PIC1DP_ERR_COMM after a time-out */
int pic1dp_hip_xchg_info(pic1dp_ctx *ctx, int32_t *memkind, int64_t *exchanges);
/* device time spent INSIDE the exchanges (the stores into the peers' slots, the wait for
 * their flags, the rank-order sum) of the launches enqueued while the timers were on
 * (pic1dp_hip_timers_enable), from a 100 MHz wall clock read in the kernel: with the
 * exchange being the prologue of the field solve's launch, this is what splits the
 * reference's "mpiallredu" share (src/pic1dp_global.F90:38-50, timer 21) from "field
 * electric" (7) in that launch.  reset != 0: start over.  Synchronises the stream. */
int pic1dp_hip_xchg_time(pic1dp_ctx *ctx, double *ms, int64_t *exchanges_timed, int32_t reset);

/* ---- timers: accumulated milliseconds under the reference's timer ids
 * (src/pic1dp_global.F90:38-50), measured with HIP events on the stream.
 * timers_enable(on): 0 off; 1 every launch is bracketed by an event pair (exact; each
 * pair costs the stream ~3 us of dependency -- 10-28 % of a 70 us time step at the
 * reference's default size); n >= 2: launches under a timer id are bracketed in blocks of
 * 64 consecutive ones, every n-th block (inside a block as with on = 1, so that a run's
 * output steps and plain steps enter in their own proportions); the others are counted, and
 * pic1dp_hip_timer_ms reports the timed ones scaled by launches seen / launches timed
 * (what the Fortran host asks for: n = 17: a sixteenth of the cost, the time loop of the
 * default run 0.91 s against 1.10-1.17 with on = 1 and 0.90-0.93 with the timers off). ---- */
int pic1dp_hip_timers_enable(pic1dp_ctx *ctx, int32_t on);
int pic1dp_hip_timer_ms(pic1dp_ctx *ctx, int32_t iwt, double *ms);
int pic1dp_hip_timers_reset(pic1dp_ctx *ctx);

/* ---- tuning knobs (performance only; results do not depend on them apart
 * from floating-point summation order of the charge) ----------------------- */
/* threads per workgroup (multiple of 64, <= 1024; 0 = auto) and workgroups per
 * CU (0 = auto) of the particle kernels */
int pic1dp_hip_set_launch(pic1dp_ctx *ctx, int32_t threads, int32_t blocks_per_cu);
/* opaque HIP stream handle (hipStream_t) the context enqueues on */
int pic1dp_hip_get_stream(pic1dp_ctx *ctx, void **stream);
/* name and launch counters of the particle kernels, for bench.py's roofline:
 * accumulated device milliseconds (HIP events on the context's stream) and
 * launch count of the fused push+deposit kernel (which=0), the separate push
 * kernel (1), the separate deposit kernel (2), and the whole-step kernels:
 * first sub-step k_step_half (3), second sub-step k_step_full (4); which = 5: number
 * of separate diagnostics passes (k_ptcldist) launched so far, *ms = 0; which = 6: the
 * one-pass-per-step kernel k_step_one (second sub-step + prediction of the next first
 * sub-step's charge); which = 7: number of k_step_one / k_step_sums launches so far whose
 * prologue solved the field of the previous step (one launch per time step inside
 * pic1dp_hip_step: no field_solve_electric launch in between), *ms = 0; which = 8:
 * *launches = bytes marker optimisation events (pic1dp_hip_particle_optimize) have moved
 * between host and device so far, *ms = 0; which = 9: *launches = how the serial forward
 * sums of the field solve (one-rank order, up to eight kept modes) run: 0 chains of
 * additions in single lanes, 1 through the FP64 matrix unit (only where pic1dp_hip_create
 * found it to reproduce the sequential sums bit for bit; PIC1DP_CHAIN_MFMA=0 keeps the chains),
 * *ms = that self-test's verdict (1 identical, 0 differs, -1 it could not run: the chains then);
 * which = 10: *launches = marker launches so far whose last workgroup packed this rank's charge
 * for the sum over ranks or posted it into the peers' exchange slots itself (several ranks: no
 * separate packing launch in front of the all-reduce; PIC1DP_TAIL=0 keeps that launch), *ms = 0;
 * which = 11: *launches = pic1dp_hip_solve_field calls of a first sub-step that launched nothing
 * because the solve_field before them had solved both fields in one launch (one rank, the three
 * call sites: two launches per time step; PIC1DP_CALL_PAIR=0: three), *ms = 0;
 * which = 12: *launches = diagnostics passes (k_ptcldist) whose (x, v) histograms were summed as
 * 64-bit fixed-point numbers in the LDS (1.9x the atomic rate of double sums; scaled by the
 * species' max |p|, max |w| of the pass before; PIC1DP_DIAG_FX=0: always doubles), *ms = how many
 * of them met a marker beyond those bounds and were repeated with double sums;
 * which = 13: *launches = terms of the one-pass kernel's prediction tiles (two and three kept modes: 64-bit
 * fixed-point LDS sums scaled by per-species bounds that follow the markers) that lay beyond 16x their bound and
 * were added in doubles straight into the global accumulators -- rare by design, a count that grows with every
 * step says the bounds have lost the population; *ms = the first species' bound on |q| as it stands (waits for the stream);
 * which = 14: *launches = contributions of the exact charge sum (set_charge_sum(1)) beyond 2^62 quanta so far, which
 * were not summed (each batch is reported once as PIC1DP_ERR_ARG), *ms = 0 (waits for the stream)
 * which = 15: *launches = terms the passes of the exact diagnostics sum (set_diag_sum(1)) did not sum so far (counted
 * when a pass's results are first handed out), *ms = 0;
 * which = 16: *launches = passes of pic1dp_hip_moments (k_moments) launched so far, *ms = their accumulated device
 * milliseconds while kernel stats were enabled;
 * which = 17: *launches = passes of pic1dp_hip_moments_exact / _moments_local_exact (k_moments_exact) launched so far,
 * *ms = their accumulated device milliseconds while kernel stats were enabled;
 * which = 18: *launches = terms those passes did not sum so far (2^44 quanta or more, or NaN; each call that met some
 * returned PIC1DP_ERR_ARG), *ms = 0;
 * which = 19: *launches = passes of pic1dp_hip_particle_load_device (k_load, one per species and call) launched so far,
 * *ms = their accumulated device milliseconds while kernel stats were enabled;
 * which = 20: *launches = passes of pic1dp_hip_power (k_power) launched so far, *ms = their accumulated device
 * milliseconds while kernel stats were enabled;
 * which = 21: *launches = passes over the markers of pic1dp_hip_select_count and pic1dp_hip_select launched so far -- the
 * count pass (k_select_count, with the prefix sum of the chunk counts behind it) and the write pass (k_select_write) count
 * one each: 1 per select_count, 2 per select that hands markers out, 1 per select with nothing to write (max = 0, no
 * marker selected, or every output pointer NULL), 0 for a species without valid markers -- *ms = their accumulated device
 * milliseconds while kernel stats were enabled;
 * which = 22: *launches = launches of pic1dp_hip_gather (k_gather, one per call with n > 0) so far, *ms = their accumulated
 * device milliseconds while kernel stats were enabled.
 * The rows end at 22: the exact power's passes are reported by pic1dp_hip_power_exact_stats below. */
int pic1dp_hip_kernel_stats(pic1dp_ctx *ctx, int32_t which, double *ms,
                            int64_t *launches);
/* the exact power (pic1dp_hip_power_exact / _power_local_exact): *passes = passes of k_power_exact that swept markers so far (a
 * call refused for a field that is not finite counts none), *ms = the accumulated device milliseconds of the passes launched
 * while kernel stats were enabled, *rejected = terms those passes did not sum so far (2^44 quanta or more, or NaN; each call
 * that met some returned PIC1DP_ERR_ARG).  Any of the three pointers may be null.  (Not rows of pic1dp_hip_kernel_stats: its
 * range 0..22 is part of what callers rely on.) */
int pic1dp_hip_power_exact_stats(pic1dp_ctx *ctx, double *ms, int64_t *passes, int64_t *rejected);
int pic1dp_hip_kernel_stats_enable(pic1dp_ctx *ctx, int32_t on);
/* what the marker kernel launched last under `which` (numbering of kernel_stats; not 5)
 * moves per marker and launch, in bytes: read_bytes (x, v, p (+ w); the RK base as well
 * for the second sub-step's k_push) and written_bytes (x (+ v) (+ w)) are compulsory for
 * its data flow; carry_bytes is the traffic the kernel CHOOSES to spend on handing
 * -f0'/f0 to the next launch instead of evaluating it again (k_step_one: 8 read + 8
 * written; 0 when it recomputes).  name: the kernel (k_step_one / k_step_sums / ...) and
 * the form of -f0'/f0 it was instantiated with.  bench.py prices its roofline on these. */
int pic1dp_hip_kernel_bytes(pic1dp_ctx *ctx, int32_t which, double *read_bytes,
                            double *written_bytes, double *carry_bytes, char *name,
                            int32_t name_len);

/* Debugging aid: checks the relations between the flags of the library's internal state machine (lazy call sites,
 * prediction, call-site pair, accumulator sets: DESIGN.md 0) that have to hold between any two calls, whatever the
 * calls were.  deep != 0 also synchronises and looks at device memory (accumulator sets nobody owes anything to are
 * zero).  PIC1DP_ERR_STATE + pic1dp_hip_last_error() name the relation that does not hold.  Replaces nothing in the
 * reference; the randomised call-sequence tests call it after every call. */
int pic1dp_hip_check_state(pic1dp_ctx *ctx, int32_t deep);

#ifdef __cplusplus
}
#endif
#endif /* PIC1DP_HIP_H */
