"""Host-side mirror of the reference's module procedures for the time-step hot
path, on top of the C ABI (include/pic1dp_hip.h).

Method names are the reference's procedure names so that a parity test reads
like the reference driver (src/pic1dp.F90:64-109):

    sim = Pic1dp(make_input(nparticle_max=10**7, nx=256))
    sim.particle_load()
    sim.interaction_collect_charge(); sim.field_solve_electric()
    for irk in (1, 2):
        sim.interaction_push_particle(irk)
        sim.interaction_collect_charge(); sim.field_solve_electric()

All compute runs in hand-written HIP kernels on one MI355X; nothing here
computes, and there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import Hermite, Input, Layout, Pic1dpError, Select, Zoom, check  # noqa: F401


def make_input(**kw):
    """pic1dp_input with the reference's default input file
    (src/pic1dp_input.F90) except multirand_seed_type=1; keyword names are the
    reference names without the input_ prefix.  Array-valued parameters take
    sequences."""
    L = _lib.load()
    inp = Input()
    check(L.pic1dp_hip_input_defaults(C.byref(inp)))
    names = {n for n, _ in Input._fields_}
    explicit_init = "species_nparticle_init" in kw
    for k, val in kw.items():
        if k not in names or k == "abi_version":
            raise KeyError("unknown input parameter %r" % k)
        cur = getattr(inp, k)
        if hasattr(cur, "__len__"):
            if len(val) > len(cur):
                raise ValueError("%s: at most %d entries" % (k, len(cur)))
            for i, x in enumerate(val):
                cur[i] = x
        else:
            setattr(inp, k, val)
    if not explicit_init:
        # input_species_nparticle_init = input_nparticle_max (src/pic1dp_input.F90:117)
        for s in range(max(0, min(inp.nspecies, _lib.MAX_SPECIES))):
            inp.species_nparticle_init[s] = inp.nparticle_max
    # marker-optimisation lists not given: the reference's implied-do formulas of the
    # counts (src/pic1dp_input.F90:149-158, 165-180, 191-200)
    for kind in ("merge", "remove", "split"):
        n = max(0, min(getattr(inp, "n" + kind), _lib.MAX_OPT))
        if "t" + kind not in kw:
            for i in range(1, n + 1):
                getattr(inp, "t" + kind)[i - 1] = 50.0 + i * 0.5
        if "thsh" + kind not in kw:
            for i in range(1, n + 1):
                val = 1.0 - 0.9 / max(n, 1) * float(i) if kind == "split" else 0.1 / max(n, 1) * float(i)
                getattr(inp, "thsh" + kind)[i - 1] = val
    return inp


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Pic1dp:
    """one process = one GPU = one context"""

    def __init__(self, inp, rank=0, nranks=1, npe=0, device=-1):
        self.L = _lib.load()
        self.inp = inp
        self.rank, self.nranks = rank, nranks
        self.npe = npe or nranks
        self._ctx = C.c_void_p()
        lay = Layout(rank, nranks, self.npe, device)
        check(self.L.pic1dp_hip_create(C.byref(inp), C.byref(lay), C.byref(self._ctx)))

    # -- life cycle (particle_final / field_final) ---------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self.L.pic1dp_hip_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- sizes -----------------------------------------------------------------
    def local_sizes(self, ispecies=0):
        na, npv = C.c_int64(), C.c_int64()
        check(self.L.pic1dp_hip_local_sizes(self._ctx, ispecies, C.byref(na), C.byref(npv)))
        return na.value, npv.value

    # -- particle_load (src/pic1dp_particle.F90:145-269) -----------------------
    def particle_load(self):
        check(self.L.pic1dp_hip_particle_load(self._ctx))

    def particle_load_device(self, kind=2):
        """the initial condition made on the GPU, every marker a function of its global index (so the same markers whatever
        npe and nranks): kind 1 counter-based random, 2 quiet start (bit-reversed v, base-3 reversed x)"""
        check(self.L.pic1dp_hip_particle_load_device(self._ctx, int(kind)))

    def set_seed_offset(self, offset):
        """ensemble member: reference block b of the next particle_load draws from RNG stream mype = b + offset
        (0: the reference's constant-seed run)"""
        check(self.L.pic1dp_hip_set_seed_offset(self._ctx, int(offset)))

    def particles_upload(self, x, v, p, w, ispecies=0, np_valid=None):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, v, p, w)]
        n = arrs[0].size
        if any(a.size != n for a in arrs):
            raise ValueError("x, v, p, w must have one length")
        check(self.L.pic1dp_hip_particles_upload(
            self._ctx, ispecies, *[_ptr(a) for a in arrs], n, n if np_valid is None else np_valid))

    def particles_download(self, ispecies=0):
        n, _ = self.local_sizes(ispecies)
        out = [np.empty(n) for _ in range(4)]
        check(self.L.pic1dp_hip_particles_download(self._ctx, ispecies, *[_ptr(a) for a in out], n))
        return dict(zip("xvpw", out))

    def particles_download_bak(self, ispecies=0):
        n, npv = self.local_sizes(ispecies)
        out = [np.zeros(n) for _ in range(3)]
        check(self.L.pic1dp_hip_particles_download_bak(self._ctx, ispecies, *[_ptr(a) for a in out], n))
        return dict(zip(("xb", "vb", "wb"), [a[:npv] for a in out]))

    # -- velocity moments on the field grid ---------------------
    def moments(self, ispecies=0, which=3):
        """sum q v^k, k = 0 ... 3, of a species' markers on the nx cells of the field grid, with the deposit's linear
        weights, computed on the GPU (include/pic1dp_hip.h pic1dp_hip_moments).  which: 1 the weights p (total f), 2 the
        weights w (delta f), 3 both.  Returns {"total": (4, nx), "pertb": (4, nx)} with only the sets asked for; row k is
        the power of v.  The sums are raw and local to this context (ranks: add element by element): density
        n = M[0] nx / lx, current J = Z M[1] nx / lx, second moment m M[2] nx / lx, third moment m M[3] nx / lx; "pertb"[0]
        is the species' deposited charge before Z nx / lx.  Markers beyond v_max count; tail slots do not.  Between time
        steps the call changes nothing; inside one it first puts a noted push into memory."""
        nx = self.inp.nx
        nsets = 2 if which == 3 else 1
        out = np.empty((nsets, 4, nx))
        check(self.L.pic1dp_hip_moments(self._ctx, int(ispecies), int(which), _ptr(out)))
        names = [n for bit, n in ((1, "total"), (2, "pertb")) if which & bit]
        return {n: out[j] for j, n in enumerate(names)}

    # -- exact, order-independent velocity moments ---------------
    def moments_exact(self, ispecies=0, which=3):
        """moments() with integer sums (include/pic1dp_hip.h pic1dp_hip_moments_exact): every term rounded once to whole
        quanta 2^e[k] (moments_quanta), the integers summed exactly, every bin converted once.  The same dict as moments();
        fixed by the input and the markers alone.  Pic1dpError naming species, weight set and power if a term lay at or
        beyond 2^44 quanta (kernel_stats(18) counts them)."""
        nsets = 2 if which == 3 else 1
        out = np.empty((nsets, 4, self.inp.nx))
        check(self.L.pic1dp_hip_moments_exact(self._ctx, int(ispecies), int(which), _ptr(out)))
        names = [n for bit, n in ((1, "total"), (2, "pertb")) if which & bit]
        return {n: out[j] for j, n in enumerate(names)}

    def moments_local_exact(self, ispecies=0, which=3):
        """this context's exact sums as int64 limbs of shape (nsets, 4, 2, nx): [j, k, 0] the hi limb, [j, k, 1] the lo limb,
        normalised (0 <= lo < 2^32); a bin's total is hi 2^32 + lo quanta.  Ranks: add element by element, then
        moments_convert"""
        nsets = 2 if which == 3 else 1
        out = np.zeros((nsets, 4, 2, self.inp.nx), dtype=np.int64)
        check(self.L.pic1dp_hip_moments_local_exact(self._ctx, int(ispecies), int(which), _ptr(out)))
        return out

    # -- velocity-resolved wave-particle power on the output grid --
    def power(self, ispecies=0, which=3):
        """the power the field does on a species' markers, q v E(x) per marker, on the nx_opd x nv_opd output grid, computed
        on the GPU (include/pic1dp_hip.h pic1dp_hip_power).  which: 1 the weights p (total f), 2 the weights w (delta f),
        3 both.  Returns {"total": {"xv": (nv_opd, nx_opd), "v": (nv_opd,), "rest": float}, "pertb": {...}} with only the
        sets asked for: "xv" the plane, "v" its sum over x, "rest" the sum over the markers with |v| >= v_max, which have no
        bins.  The sums are raw and local to this context (ranks: add element by element); species_charge * t is the rate
        of work on the marker's share of f or delta f."""
        n = C.c_int64()
        check(self.L.pic1dp_hip_power_len(C.byref(self.inp), int(which), C.byref(n)))
        out = np.zeros(n.value)
        check(self.L.pic1dp_hip_power(self._ctx, int(ispecies), int(which), _ptr(out)))
        return _split_power(out, self.inp, which)

    # -- exact, order-independent wave-particle power -------------
    def power_exact(self, ispecies=0, which=3):
        """power() with integer sums (include/pic1dp_hip.h pic1dp_hip_power_exact): every term rounded once to whole quanta
        2^e, e from the input and max |E| of the call (power_quantum), the integers summed exactly, every bin converted
        once, "v" the exact integer row sums.  The same dict as power(); fixed by the input, the markers and the field
        alone.  Pic1dpError if the field is not finite, or naming species, weight set and bins or rest if a term lay at or
        beyond 2^44 quanta (power_exact_stats counts them)."""
        n = C.c_int64()
        check(self.L.pic1dp_hip_power_len(C.byref(self.inp), int(which), C.byref(n)))
        out = np.zeros(n.value)
        check(self.L.pic1dp_hip_power_exact(self._ctx, int(ispecies), int(which), _ptr(out)))
        return _split_power(out, self.inp, which)

    def power_exact_stats(self):
        """(device ms of the exact power's passes while kernel stats were enabled, passes that swept markers so far, terms
        they did not sum so far) -- pic1dp_hip_power_exact_stats; kernel_stats has no row for them"""
        ms, n, rej = C.c_double(), C.c_int64(), C.c_int64()
        check(self.L.pic1dp_hip_power_exact_stats(self._ctx, C.byref(ms), C.byref(n), C.byref(rej)))
        return ms.value, n.value, rej.value

    def power_local_exact(self, ispecies=0, which=3):
        """(limbs, log2_quantum): this context's exact sums as int64 limbs of shape (nsets, 2 nx_opd nv_opd + 2) -- per set
        [hi plane | lo plane | rest hi | rest lo], normalised (0 <= lo < 2^32), a total is hi 2^32 + lo quanta -- and the e of
        the call.  Ranks: check that e agrees, add the limbs element by element, then power_convert"""
        limbs = np.zeros((2 if which == 3 else 1, power_limbs_len(self.inp, which) // (2 if which == 3 else 1)), dtype=np.int64)
        e = C.c_int32()
        check(self.L.pic1dp_hip_power_local_exact(self._ctx, int(ispecies), int(which), _ptr(limbs), C.byref(e)))
        return limbs, e.value

    # -- exact phase-space histogram on a caller-chosen window and grid --
    def zoom(self, ispecies=0, x=None, v=None, bins=(64, 64), which=7):
        """the markers of a species counted, and their p and w summed, on a cell-centred grid of bins = (nxb, nvb) cells over
        the window x = (lo, hi) of the wrapped position (lo > hi: across the periodic boundary; None: the whole box) and
        v = (lo, hi) (None: [-v_max, v_max)), on the GPU (include/pic1dp_hip.h pic1dp_hip_zoom).  which: a mask of 1 markr,
        2 total, 4 pertb.  Returns a dict of the planes asked for as (nvb, nxb) arrays, plus x_edges (nxb + 1, running past
        lx where the window straddles) and v_edges (nvb + 1).  Exact: every term rounded once to whole quanta and summed as
        integers, so the result is fixed by the input and the markers alone.  The sums are raw and local to this context;
        divide by the cell's area for a density.  Pic1dpError naming species and plane if a term lay at or beyond 2^44
        quanta (zoom_stats counts them)."""
        z = make_zoom(self.inp, x, v, bins)
        out = np.zeros((_zoom_planes(which),) + _zoom_shape(z))
        check(self.L.pic1dp_hip_zoom(self._ctx, int(ispecies), C.byref(z), int(which), _ptr(out)))
        return _split_zoom(out, self.inp, z, which)

    def hermite(self, ispecies=0, modes=(1,), nherm=64, v0=0.0, vt=1.0, which=3):
        """the Fourier-Hermite spectrum g_{k,n} = sum_i q_i psi_n((v_i - v0) / vt) exp(-i k x_i) of a species' markers for
        the Fourier modes `modes` and n < nherm, summed on the GPU's FP64 matrix unit (include/pic1dp_hip.h
        pic1dp_hip_hermite).  which: 1 the weights p (total f), 2 the weights w (delta f), 3 both.  Returns {"total":
        complex128 (nmodes, nherm), "pertb": ...} with only the sets asked for, each entry C - iS: the coefficient of
        exp(+ikx) psi_n(u) exp(-u^2 / 2) / sqrt(2 pi).  |g|^2 against n is the free-energy spectrum of the mode.  The sums
        are raw and local to this context (ranks: add element by element).  Between time steps the call changes nothing;
        inside one it first puts a noted push into memory."""
        h = make_hermite(modes, nherm, v0, vt)
        out = np.zeros(_hermite_shape(h, which))
        check(self.L.pic1dp_hip_hermite(self._ctx, int(ispecies), int(which), C.byref(h), _ptr(out)))
        return _split_hermite(out, which)

    def hermite_stats(self):
        """(device ms of the spectrum's passes while kernel stats were enabled, passes launched so far) --
        pic1dp_hip_hermite_stats; kernel_stats has no row for them"""
        ms, n = C.c_double(), C.c_int64()
        check(self.L.pic1dp_hip_hermite_stats(self._ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def zoom_local_exact(self, ispecies=0, x=None, v=None, bins=(64, 64), which=7):
        """this context's exact sums as int64 limbs of shape (nplanes, 2, nvb, nxb): [j, 0] the hi limb, [j, 1] the lo limb,
        normalised (0 <= lo < 2^32); a cell's total is hi 2^32 + lo quanta.  Ranks: add element by element, then zoom_convert"""
        z = make_zoom(self.inp, x, v, bins)
        limbs = np.zeros((_zoom_planes(which), 2) + _zoom_shape(z), dtype=np.int64)
        check(self.L.pic1dp_hip_zoom_local_exact(self._ctx, int(ispecies), C.byref(z), int(which), _ptr(limbs)))
        return limbs

    def zoom_stats(self):
        """(device ms of the zoom's passes while kernel stats were enabled, passes that swept markers so far, terms they did
        not sum so far) -- pic1dp_hip_zoom_stats; kernel_stats has no row for them"""
        ms, n, rej = C.c_double(), C.c_int64(), C.c_int64()
        check(self.L.pic1dp_hip_zoom_stats(self._ctx, C.byref(ms), C.byref(n), C.byref(rej)))
        return ms.value, n.value, rej.value

    # -- select and gather markers on the GPU --------------------
    def _selection(self, ispecies, x, v, fraction, key, origin):
        if origin is None:
            origin = load_origin(self.inp, ispecies, self.rank, self.nranks, self.npe)
        return make_select(x, v, fraction, key, origin)

    def select_count(self, ispecies=0, x=(-np.inf, np.inf), v=(-np.inf, np.inf), fraction=1.0, key=0, origin=None):
        """how many valid markers of a species select() would hand out (include/pic1dp_hip.h pic1dp_hip_select_count): one
        pass over x and v on the GPU, nothing but the count crosses to the host"""
        sel, n = self._selection(int(ispecies), x, v, fraction, key, origin), C.c_int64()
        check(self.L.pic1dp_hip_select_count(self._ctx, int(ispecies), C.byref(sel), C.byref(n)))
        return n.value

    def select(self, ispecies=0, x=(-np.inf, np.inf), v=(-np.inf, np.inf), fraction=1.0, key=0, origin=None, max=None):
        """the valid markers of a species inside a window, thinned by a hash of their global index, selected and compacted
        on the GPU (include/pic1dp_hip.h pic1dp_hip_select).  x = (lo, hi): lo <= wrap(x) < hi, or the window across the
        periodic boundary when lo > hi; v = (lo, hi): lo <= v < hi; +-inf says "all".  fraction: the share of the
        window's markers to keep, the same markers at every time (a tracer set) and, with origin = this context's
        load_origin (the default, None), the same markers however the run is split over ranks.  Returns dict(count, index,
        x, v, p, w) in ascending logical index: `count` is the number selected, the arrays hold the first min(count, max)
        of them (max=None: all -- it counts first and sizes the arrays from the count); x is as stored, not wrapped."""
        isp = int(ispecies)
        sel, n = self._selection(isp, x, v, fraction, key, origin), C.c_int64()
        if max is None:
            check(self.L.pic1dp_hip_select_count(self._ctx, isp, C.byref(sel), C.byref(n)))
            max = n.value
        index = np.empty(int(max), dtype=np.int64)
        out = [np.empty(int(max)) for _ in range(4)]
        check(self.L.pic1dp_hip_select(self._ctx, isp, C.byref(sel), int(max), C.byref(n), _ptr(index), *[_ptr(a) for a in out]))
        m = min(n.value, int(max))
        res = {"count": n.value, "index": index[:m]}
        res.update({k: a[:m] for k, a in zip("xvpw", out)})
        return res

    def gather(self, ispecies, index):
        """x, v, p, w of the markers at the given logical indices (any order, duplicates allowed, tail slots included), read
        on the GPU (include/pic1dp_hip.h pic1dp_hip_gather): dict(x, v, p, w), equal to particles_download()[..][index]"""
        idx = np.ascontiguousarray(index, dtype=np.int64).ravel()
        out = [np.empty(idx.size) for _ in range(4)]
        check(self.L.pic1dp_hip_gather(self._ctx, int(ispecies), _ptr(idx), idx.size, *[_ptr(a) for a in out]))
        return dict(zip("xvpw", out))

    # -- state digest, checkpoint and restart -----------------
    def state_digest(self):
        """D[s][k] of the markers on the device (include/pic1dp_hip.h): uint64 [nspecies][4], k = 0 x, 1 v, 2 w, 3 p;
        equals host_digest() of what particles_download() returns, array by array"""
        out = np.zeros((self.inp.nspecies, 4), dtype=np.uint64)
        check(self.L.pic1dp_hip_state_digest(self._ctx, _ptr(out)))
        return out

    def checkpoint_write(self, path):
        """everything that decides later bits into one file (only between time steps); afterwards this context and one
        restored from the file continue bit for bit alike -- the next step takes two passes"""
        check(self.L.pic1dp_hip_checkpoint_write(self._ctx, os.fsencode(path)))

    def checkpoint_read(self, path):
        """restore from a file written by a context of the same input, layout and settings"""
        check(self.L.pic1dp_hip_checkpoint_read(self._ctx, os.fsencode(path)))

    SETTING_NAMES = ("charge_sum", "diag_sum", "field_transform", "field_solver", "step_mode", "fuse_output", "seed_offset")

    def apply_settings(self, settings):
        """the seven settings a checkpoint carries (checkpoint_info()["settings"]), through their own calls"""
        self.set_seed_offset(settings["seed_offset"])
        self.set_step_mode(settings["step_mode"])
        check(self.L.pic1dp_hip_set_output_fusion(self._ctx, int(settings["fuse_output"])))
        self.set_field_solver(settings["field_solver"])
        self.set_field_transform(settings["field_transform"])
        self.set_charge_sum(settings["charge_sum"])
        self.set_diag_sum(settings["diag_sum"])

    @classmethod
    def from_checkpoint(cls, path, device=-1):
        """a fresh context from the file's input and layout, with its seven settings, holding its state"""
        info = checkpoint_info(path)
        sim = cls(info["input"], rank=info["rank"], nranks=info["nranks"], npe=info["npe"], device=device)
        try:
            sim.apply_settings(info["settings"])
            sim.checkpoint_read(path)
        except Exception:
            sim.close()
            raise
        return sim

    # -- the hot path, under the reference's names -----------------------------
    def interaction_collect_charge(self):
        check(self.L.pic1dp_hip_collect_charge(self._ctx))

    def field_solve_electric(self):
        check(self.L.pic1dp_hip_solve_field(self._ctx))

    def interaction_push_particle(self, irk):
        check(self.L.pic1dp_hip_push(self._ctx, irk))

    def particle_optimize(self, irk=2):
        """particle_optimize (src/pic1dp_particle.F90:724-783) after the push of
        sub-step irk; True when a merge / remove / split was performed"""
        flag = C.c_int32()
        check(self.L.pic1dp_hip_particle_optimize(self._ctx, irk, C.byref(flag)))
        return bool(flag.value)

    def substep(self, irk):
        """push(irk) + collect_charge + solve_field, push and deposit fused"""
        check(self.L.pic1dp_hip_substep(self._ctx, irk))

    def step(self, nsteps=1):
        check(self.L.pic1dp_hip_step(self._ctx, nsteps))

    def sync(self):
        check(self.L.pic1dp_hip_sync(self._ctx))

    def set_step_mode(self, mode):
        """0: whole-step kernels (half-step state recomputed, default);
        1: two fused sub-steps through the RK ping-pong sets"""
        check(self.L.pic1dp_hip_set_step_mode(self._ctx, mode))

    def chargeden_kept_mode_only(self):
        """True: field_chargeden holds only the kept mode's content of the half-step charge density (between the
        sub-steps of a step whose half-step charge was predicted as six sums, where the library could not rebuild the
        reference's vector: several ranks); False: it is the reference's vector"""
        k = C.c_int32()
        check(self.L.pic1dp_hip_chargeden_state(self._ctx, C.byref(k)))
        return bool(k.value)

    def predict_kind(self):
        """how step mode 0 predicts the next first sub-step's charge: 0 not (two passes per step),
        1 prediction tiles (k_step_one), 2 six sums (k_step_sums, large grids)"""
        k = C.c_int32(0)
        check(self.L.pic1dp_hip_predict_kind(self._ctx, C.byref(k)))
        return k.value

    def set_output_fusion(self, on=True):
        """diagnostics of output_all taken inside the step that precedes it: False / 0 never, True / 1 where it pays
        (not on a predicted one-pass step, whose prediction k_step_full<DIAG> would cost), 2 always"""
        check(self.L.pic1dp_hip_set_output_fusion(self._ctx, int(on)))

    def set_field_solver(self, kind):
        """0: the reference's mode-filter solve (default); 1: opt-in finite-difference
        tridiagonal solve by parallel cyclic reduction (not in the reference)"""
        check(self.L.pic1dp_hip_set_field_solver(self._ctx, kind))

    def set_field_transform(self, kind):
        """how the mode-filter solve computes its DFT: 0 the direct partial DFT against dense tables (default, the
        reference's sums); 1 an FFT (for many kept modes; nx = 2^a 3^b 5^c, see field_transform_supported)"""
        check(self.L.pic1dp_hip_set_field_transform(self._ctx, int(kind)))

    def get_field_half(self):
        """field_electric between the two sub-steps of the last step()"""
        E = np.empty(self.inp.nx)
        check(self.L.pic1dp_hip_get_field_half(self._ctx, _ptr(E)))
        return E

    # -- driver scalars (global_itime, global_time) -----------------------------
    @property
    def itime(self):
        it, t = C.c_int32(), C.c_double()
        check(self.L.pic1dp_hip_get_time(self._ctx, C.byref(it), C.byref(t)))
        return it.value

    @property
    def time(self):
        it, t = C.c_int32(), C.c_double()
        check(self.L.pic1dp_hip_get_time(self._ctx, C.byref(it), C.byref(t)))
        return t.value

    def set_time(self, itime, time):
        check(self.L.pic1dp_hip_set_time(self._ctx, itime, time))

    def check_termination(self):
        f = C.c_int32()
        check(self.L.pic1dp_hip_check_termination(self._ctx, C.byref(f)))
        return f.value

    def output_due(self, itermination=0):
        f = C.c_int32()
        check(self.L.pic1dp_hip_output_due(self._ctx, itermination, C.byref(f)))
        return f.value

    def steps_to_output(self):
        """iterations of the driver loop (src/pic1dp.F90:78-109) up to and including the one output_all follows"""
        n = C.c_int32()
        check(self.L.pic1dp_hip_steps_to_output(self._ctx, C.byref(n)))
        return n.value

    def check_state(self, deep=True):
        """debugging aid: the relations between the flags of the library's state machine that hold between any two
        calls; deep also looks at the device's accumulator sets.  Raises Pic1dpError naming the
        relation that does not hold."""
        check(self.L.pic1dp_hip_check_state(self._ctx, 1 if deep else 0))

    # -- field access -------------------------------------------------------------
    def get_field(self, chargeden=True):
        """field_electric, field_chargeden, field_mode_re / _im (src/pic1dp_field.F90:27-31).  chargeden=False
        leaves field_chargeden alone (no key in the result): asking for it between the sub-steps of a step
        whose half-step charge was predicted as six sums makes the library push the half-step state into
        memory and deposit it after all -- the reference's vector, at the price of that step's short cut"""
        nx, nm = self.inp.nx, self.inp.nmode
        E, re, im = np.empty(nx), np.empty(nm), np.empty(nm)
        cd = np.empty(nx) if chargeden else None
        check(self.L.pic1dp_hip_get_field(self._ctx, _ptr(E), _ptr(cd) if chargeden else None, _ptr(re), _ptr(im)))
        out = dict(electric=E, mode_re=re, mode_im=im)
        if chargeden:
            out["chargeden"] = cd
        return out

    def set_electric(self, E):
        E = np.ascontiguousarray(E, dtype=np.float64)
        if E.size != self.inp.nx:
            raise ValueError("E must have nx entries")
        check(self.L.pic1dp_hip_set_electric(self._ctx, _ptr(E)))

    def set_chargeden(self, cd):
        cd = np.ascontiguousarray(cd, dtype=np.float64)
        if cd.size != self.inp.nx:
            raise ValueError("chargeden must have nx entries")
        check(self.L.pic1dp_hip_set_chargeden(self._ctx, _ptr(cd)))

    def field_energy(self):
        e = C.c_double()
        check(self.L.pic1dp_hip_field_energy(self._ctx, C.byref(e)))
        return e.value

    def energy_history(self):
        cnt = C.c_int64()
        check(self.L.pic1dp_hip_energy_history(self._ctx, None, 0, C.byref(cnt)))
        out = np.empty(cnt.value)
        if cnt.value:
            check(self.L.pic1dp_hip_energy_history(self._ctx, _ptr(out), cnt.value, C.byref(cnt)))
        return out

    def energy_history_reset(self):
        check(self.L.pic1dp_hip_energy_history_reset(self._ctx))

    def energy_sums(self, ispecies=0):
        out = np.empty(3)
        check(self.L.pic1dp_hip_energy_sums(self._ctx, ispecies, _ptr(out)))
        return out

    def cell_indices(self, ispecies=0, want_ix=True):
        """cell of every valid marker and markers per cell (want_ix=False: the counts only -- no host array per marker)"""
        _, npv = self.local_sizes(ispecies)
        ix = np.empty(npv, dtype=np.int32) if want_ix else None
        cnt = np.empty(self.inp.nx, dtype=np.int64)
        check(self.L.pic1dp_hip_cell_indices(self._ctx, ispecies, _ptr(ix) if want_ix else None, _ptr(cnt)))
        return ix, cnt

    # -- diagnostics of output_all (src/pic1dp_output.F90) ------------------------
    def output_scalars(self):
        """realbuf of output_field: time, int E^2 dx, then 3 sums per species"""
        n = 2 + 3 * self.inp.nspecies
        out = np.empty(n)
        check(self.L.pic1dp_hip_output_scalars(self._ctx, _ptr(out), n))
        return out

    def ptcldist(self, ispecies=0, finish=True):
        """(x,v) and v distributions of output_ptcldist, computed on the GPU"""
        nxo, nvo = self.inp.nx_opd, self.inp.nv_opd
        names = ("markr_xv", "total_xv", "pertb_xv", "markr_v", "total_v", "pertb_v")
        out = [np.empty(nxo * nvo) for _ in range(3)] + [np.empty(nvo) for _ in range(3)]
        check(self.L.pic1dp_hip_ptcldist(self._ctx, ispecies, int(finish), *[_ptr(a) for a in out]))
        return dict(zip(names, out))

    def output_all(self):
        """everything output_all writes in one call and one wait: (scalars, field dict, [per-species ptcldist dicts])"""
        inp = self.inp
        ns, nx, nm = inp.nspecies, inp.nx, inp.nmode
        nxv, nvo = inp.nx_opd * inp.nv_opd, inp.nv_opd
        ntot = 3 * nxv + 3 * nvo
        scal = np.empty(2 + 3 * ns)
        E, cd, re, im = np.empty(nx), np.empty(nx), np.empty(nm), np.empty(nm)
        dist = np.empty(ns * ntot)
        check(self.L.pic1dp_hip_output_all(self._ctx, _ptr(scal), scal.size, _ptr(E), _ptr(cd), _ptr(re), _ptr(im), _ptr(dist)))
        names = ("markr_xv", "total_xv", "pertb_xv", "markr_v", "total_v", "pertb_v")
        per = []
        for s in range(ns):
            d = dist[s * ntot:(s + 1) * ntot]
            parts = [d[0:nxv], d[nxv:2 * nxv], d[2 * nxv:3 * nxv], d[3 * nxv:3 * nxv + nvo], d[3 * nxv + nvo:3 * nxv + 2 * nvo],
                     d[3 * nxv + 2 * nvo:]]
            per.append(dict(zip(names, parts)))
        return scal, dict(electric=E, chargeden=cd, mode_re=re, mode_im=im), per

    # -- split-phase diagnostics (a host that owns the reductions) --------------------
    def output_scalars_from(self, sums):
        """realbuf of output_field from the kinetic sums (energy_sums per species) summed over ranks"""
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        n = 2 + 3 * self.inp.nspecies
        out = np.empty(n)
        check(self.L.pic1dp_hip_output_scalars_from(self._ctx, _ptr(sums), _ptr(out), n))
        return out

    def ptcldist_finish(self, raw, ispecies=0):
        """ptcldist(finish=False) summed over ranks -> what output_ptcldist writes"""
        names = ("markr_xv", "total_xv", "pertb_xv", "markr_v", "total_v", "pertb_v")
        out = [np.array(raw[k], dtype=np.float64).ravel().copy() for k in names]
        check(self.L.pic1dp_hip_ptcldist_finish(self._ctx, ispecies, *[_ptr(a) for a in out]))
        return dict(zip(names, out))

    # -- split-phase deposit -------------------------------------------------------
    def charge_local(self):
        out = np.empty(self.inp.nx)
        check(self.L.pic1dp_hip_charge_local(self._ctx, _ptr(out)))
        return out

    def charge_reduced(self, charge1):
        a = np.ascontiguousarray(charge1, dtype=np.float64)
        if a.size != self.inp.nx:
            raise ValueError("charge must have nx entries")
        check(self.L.pic1dp_hip_charge_reduced(self._ctx, _ptr(a)))

    # -- exact charge sum (kind 1, include/pic1dp_hip.h) -------------------------------
    def set_charge_sum(self, kind):
        """0: FP64 atomics (default); 1: exact -- contributions rounded once to whole quanta 2^e_s and summed as
        integers, so the charge does not depend on the order of the sum.  Only between time steps."""
        check(self.L.pic1dp_hip_set_charge_sum(self._ctx, int(kind)))

    def charge_quantum(self, ispecies=0):
        """e_s of species ispecies' quantum 2^e_s in the exact charge sum (from the input alone)"""
        return charge_quantum(self.inp, ispecies)

    def charge_local_exact(self):
        """kind 1 split phase: this rank's exact deposit as int64 limbs [nspecies][2][nx] (hi, lo; lo < 2^32), to be
        summed element by element over the ranks and handed to charge_reduced_exact"""
        out = np.empty((self.inp.nspecies, 2, self.inp.nx), dtype=np.int64)
        check(self.L.pic1dp_hip_charge_local_exact(self._ctx, _ptr(out)))
        return out

    def charge_reduced_exact(self, limbs):
        a = np.ascontiguousarray(limbs, dtype=np.int64)
        if a.size != 2 * self.inp.nspecies * self.inp.nx:
            raise ValueError("limbs must have nspecies * 2 * nx entries")
        check(self.L.pic1dp_hip_charge_reduced_exact(self._ctx, _ptr(a)))

    # -- exact diagnostics sum (kind 1, include/pic1dp_hip.h) ---------------------------
    def set_diag_sum(self, kind):
        """0: the diagnostics pass as it was (default); 1: exact -- every term of the histograms and kinetic sums
        rounded once to whole quanta (diag_quanta) and summed as integers, so energy_sums, output_scalars, ptcldist
        and output_all do not depend on the order of the sums.  Only between time steps."""
        check(self.L.pic1dp_hip_set_diag_sum(self._ctx, int(kind)))

    def diag_quanta(self, ispecies=0):
        """the six log2 quanta of species ispecies (markr, total, pertb, sum v^2, sum v^2 p, sum v^2 w)"""
        return diag_quanta(self.inp, ispecies)

    def diag_limbs_len(self):
        n = C.c_int64()
        check(self.L.pic1dp_hip_diag_limbs_len(self._ctx, C.byref(n)))
        return n.value

    def diag_local_exact(self, ispecies=0):
        """kind 1 split phase: this rank's exact diagnostics sums of a species as int64 limbs, [3 planes][2][nx_opd
        nv_opd] (hi, lo) then [3 sums][2]; to be summed element by element over the ranks and handed to
        diag_convert_exact"""
        out = np.empty(self.diag_limbs_len(), dtype=np.int64)
        check(self.L.pic1dp_hip_diag_local_exact(self._ctx, int(ispecies), _ptr(out)))
        return out

    def diag_convert_exact(self, limbs, ispecies=0):
        """(sums, raw): the rank-summed limbs as energy_sums and ptcldist(finish=False) return them"""
        a = np.ascontiguousarray(limbs, dtype=np.int64)
        if a.size != self.diag_limbs_len():
            raise ValueError("limbs must have 6 * nx_opd * nv_opd + 6 entries")
        nxv, nvo = self.inp.nx_opd * self.inp.nv_opd, self.inp.nv_opd
        sums, dist = np.empty(3), np.empty(3 * nxv + 3 * nvo)
        check(self.L.pic1dp_hip_diag_convert_exact(self._ctx, int(ispecies), _ptr(a), _ptr(sums), _ptr(dist)))
        return sums, _split_dist(dist, nxv, nvo)

    # -- RCCL ------------------------------------------------------------------------
    def comm_unique_id(self):
        buf = (C.c_ubyte * _lib.COMM_ID_BYTES)()
        check(self.L.pic1dp_hip_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, uid):
        if len(uid) != _lib.COMM_ID_BYTES:
            raise ValueError("unique id must be %d bytes" % _lib.COMM_ID_BYTES)
        buf = (C.c_ubyte * _lib.COMM_ID_BYTES).from_buffer_copy(uid)
        check(self.L.pic1dp_hip_comm_init(self._ctx, buf))

    def comm_available(self):
        """raises unless librccl can be loaded in this process"""
        check(self.L.pic1dp_hip_comm_available())

    # -- one-hop charge exchange (alternative to the RCCL all-reduce) ---------------
    def xchg_create(self):
        buf = (C.c_ubyte * _lib.XCHG_HANDLE_BYTES)()
        check(self.L.pic1dp_hip_xchg_create(self._ctx, buf))
        return bytes(buf)

    def xchg_connect(self, handles):
        if len(handles) != _lib.XCHG_HANDLE_BYTES * self.nranks:
            raise ValueError("need %d handle bytes per rank" % _lib.XCHG_HANDLE_BYTES)
        buf = (C.c_ubyte * len(handles)).from_buffer_copy(handles)
        check(self.L.pic1dp_hip_xchg_connect(self._ctx, buf))

    def set_allreduce(self, kind):
        """0 auto (RCCL when a communicator exists), 1 RCCL, 2 one-hop exchange"""
        check(self.L.pic1dp_hip_set_allreduce(self._ctx, kind))

    def xchg_info(self):
        kind, n = C.c_int32(), C.c_int64()
        check(self.L.pic1dp_hip_xchg_info(self._ctx, C.byref(kind), C.byref(n)))
        return kind.value, n.value

    def xchg_time(self, reset=False):
        """(ms, exchanges): device time spent inside the one-hop exchanges enqueued while the timers were on (the
        stores into the peers' slots, the wait for their flags, the rank-order sum) -- what splits the charge sum
        from the field solve inside the launch they share"""
        ms, n = C.c_double(), C.c_int64()
        check(self.L.pic1dp_hip_xchg_time(self._ctx, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    # -- timers / knobs -----------------------------------------------------------------
    def timers_enable(self, on=True):
        """False / 0 off; True / 1 HIP events around every launch; n >= 2 around every n-th block of 64 launches of a timer id (scaled)"""
        check(self.L.pic1dp_hip_timers_enable(self._ctx, int(on)))

    def timer_ms(self, iwt):
        ms = C.c_double()
        check(self.L.pic1dp_hip_timer_ms(self._ctx, iwt, C.byref(ms)))
        return ms.value

    def timers_reset(self):
        check(self.L.pic1dp_hip_timers_reset(self._ctx))

    def set_launch(self, threads=0, blocks_per_cu=0):
        check(self.L.pic1dp_hip_set_launch(self._ctx, threads, blocks_per_cu))

    def kernel_stats_enable(self, on=True):
        check(self.L.pic1dp_hip_kernel_stats_enable(self._ctx, int(on)))

    def kernel_bytes(self, which=6):
        """what the marker kernel launched last under `which` (kernel_stats numbering) moves per marker and
        launch: dict(read, written, carry, name) -- read + written are compulsory for its data flow, carry
        is the traffic it chooses to spend on not evaluating -f0'/f0 again"""
        rd, wr, ca = C.c_double(), C.c_double(), C.c_double()
        name = C.create_string_buffer(64)
        check(self.L.pic1dp_hip_kernel_bytes(self._ctx, which, C.byref(rd), C.byref(wr), C.byref(ca), name, 64))
        return dict(read=rd.value, written=wr.value, carry=ca.value, name=name.value.decode())

    def kernel_stats(self, which=0):
        ms, n = C.c_double(), C.c_int64()
        check(self.L.pic1dp_hip_kernel_stats(self._ctx, which, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # -- the reference driver, src/pic1dp.F90:64-109 ---------------------------------------
    def run(self, on_output=None, max_steps=None, fused=True):
        """particle_load must have been called.  Runs the initial deposit+solve
        and the RK2 time loop until check_termination, calling
        on_output(self) at step 0 and whenever the reference would call
        output_all.  Returns the number of steps taken."""
        if on_output:
            self.set_output_fusion(True)     # output steps take their diagnostics inside the step
        self.interaction_collect_charge()
        self.field_solve_electric()
        if on_output:
            on_output(self)
        steps = 0
        term = self.check_termination()
        while term == 0 and (max_steps is None or steps < max_steps):
            if fused:          # every step up to the next output_all in one call (src/pic1dp.F90:78-109 evaluated ahead)
                n = max(1, self.steps_to_output())
                if max_steps is not None:
                    n = min(n, max_steps - steps)
                self.step(n)
                steps += n - 1
            else:
                for irk in (1, 2):
                    self.interaction_push_particle(irk)
                    self.particle_optimize(irk)            # src/pic1dp.F90:82
                    self.interaction_collect_charge()
                    self.field_solve_electric()
                self.set_time(self.itime + 1, self.time + self.inp.dt)
            steps += 1
            term = self.check_termination()
            if on_output and self.output_due(term):
                on_output(self)
        return steps


def charge_quantum(inp, ispecies=0):
    """e_s = ceil(log2 B_s) - 52 of the exact charge sum's quantum 2^e_s, B_s a bound on the species' |p| and |w|
    from the input alone (no device)"""
    e = C.c_int32()
    check(_lib.load().pic1dp_hip_charge_quantum(C.byref(inp), int(ispecies), C.byref(e)))
    return e.value


_DIST_NAMES = ("markr_xv", "total_xv", "pertb_xv", "markr_v", "total_v", "pertb_v")


def _split_dist(dist, nxv, nvo):
    parts = [dist[0:nxv], dist[nxv:2 * nxv], dist[2 * nxv:3 * nxv], dist[3 * nxv:3 * nxv + nvo],
             dist[3 * nxv + nvo:3 * nxv + 2 * nvo], dist[3 * nxv + 2 * nvo:]]
    return dict(zip(_DIST_NAMES, parts))


def diag_quanta(inp, ispecies=0):
    """the six log2 quanta of the exact diagnostics sum of a species -- markr, total, pertb, sum v^2, sum v^2 p,
    sum v^2 w -- from the input alone (no device)"""
    e = (C.c_int32 * 6)()
    check(_lib.load().pic1dp_hip_diag_quanta(C.byref(inp), int(ispecies), e))
    return list(e)


def diag_quantise(term, log2_quantum, kinetic=False):
    """n = rint(term 2^-log2_quantum) as the exact diagnostics pass forms it; Pic1dpError for a term it would not sum"""
    n = C.c_int64()
    check(_lib.load().pic1dp_hip_diag_quantise(float(term), int(log2_quantum), int(bool(kinetic)), C.byref(n)))
    return n.value


def diag_convert(inp, limbs, ispecies=0):
    """(sums, raw) from a species' limbs summed over the ranks, from the input alone (no context, no device)"""
    a = np.ascontiguousarray(limbs, dtype=np.int64)
    nxv, nvo = inp.nx_opd * inp.nv_opd, inp.nv_opd
    if a.size != 6 * nxv + 6:
        raise ValueError("limbs must have 6 * nx_opd * nv_opd + 6 entries")
    sums, dist = np.empty(3), np.empty(3 * nxv + 3 * nvo)
    check(_lib.load().pic1dp_hip_diag_convert(C.byref(inp), int(ispecies), _ptr(a), _ptr(sums), _ptr(dist)))
    return sums, _split_dist(dist, nxv, nvo)


def moments_quanta(inp, ispecies=0):
    """e[k] = kb + k ceil(log2 v_max) - 40, k = 0 ... 3, the log2 quanta of the exact moments of a species, from the input
    alone (no device); kb = charge_quantum + 52"""
    e = (C.c_int32 * 4)()
    check(_lib.load().pic1dp_hip_moments_quanta(C.byref(inp), int(ispecies), e))
    return list(e)


def moments_limbs_len(which, nx):
    """int64 words of the limbs of the exact moments: 8 nx per selected weight set"""
    n = C.c_int64()
    check(_lib.load().pic1dp_hip_moments_limbs_len(int(which), int(nx), C.byref(n)))
    return n.value


def moments_convert(inp, limbs, which=3, ispecies=0):
    """the dict of Pic1dp.moments() from limbs (nsets, 4, 2, nx) as moments_local_exact returns them, or their element-wise
    sum over ranks (lo need not be normalised), from the input alone (no context, no device)"""
    a = np.ascontiguousarray(limbs, dtype=np.int64)
    nsets = 2 if which == 3 else 1
    if a.size != nsets * 8 * inp.nx:
        raise ValueError("limbs must have 8 * nx entries per selected weight set")
    out = np.empty((nsets, 4, inp.nx))
    check(_lib.load().pic1dp_hip_moments_convert(C.byref(inp), int(ispecies), int(which), _ptr(a), _ptr(out)))
    names = [n for bit, n in ((1, "total"), (2, "pertb")) if which & bit]
    return {n: out[j] for j, n in enumerate(names)}


def _split_power(out, inp, which):
    """the dict of Pic1dp.power() from its flat output"""
    nxo, nvo = inp.nx_opd, inp.nv_opd
    per = nxo * nvo + nvo + 1
    names = [name for bit, name in ((1, "total"), (2, "pertb")) if which & bit]
    res = {}
    for j, name in enumerate(names):
        o = out[j * per:(j + 1) * per]
        res[name] = {"xv": o[:nxo * nvo].reshape(nvo, nxo).copy(), "v": o[nxo * nvo:nxo * nvo + nvo].copy(), "rest": float(o[-1])}
    return res


def power_quantum(inp, max_abs_E, ispecies=0):
    """e = max(kb + ceil(log2 v_max) + kE - 40, -1000), the log2 quantum of the exact power of a species, from the input and
    max |E| (no device); kb = charge_quantum + 52, kE = ceil(log2 max_abs_E), 0 for a field of zeros"""
    e = C.c_int32()
    check(_lib.load().pic1dp_hip_power_quantum(C.byref(inp), int(ispecies), float(max_abs_E), C.byref(e)))
    return e.value


def power_limbs_len(inp, which):
    """int64 words of the limbs of the exact power: 2 nx_opd nv_opd + 2 per selected weight set"""
    n = C.c_int64()
    check(_lib.load().pic1dp_hip_power_limbs_len(C.byref(inp), int(which), C.byref(n)))
    return n.value


def power_convert(inp, limbs, log2_quantum, which=3):
    """the dict of Pic1dp.power() from limbs (nsets, 2 nx_opd nv_opd + 2) as power_local_exact returns them, or their
    element-wise sum over ranks (lo need not be normalised), and the ranks' common log2_quantum (no context, no device)"""
    a = np.ascontiguousarray(limbs, dtype=np.int64)
    if a.size != power_limbs_len(inp, which):
        raise ValueError("limbs must have 2 * nx_opd * nv_opd + 2 entries per selected weight set")
    n = C.c_int64()
    check(_lib.load().pic1dp_hip_power_len(C.byref(inp), int(which), C.byref(n)))
    out = np.zeros(n.value)
    check(_lib.load().pic1dp_hip_power_convert(C.byref(inp), int(which), int(log2_quantum), _ptr(a), _ptr(out)))
    return _split_power(out, inp, which)


def host_digest(a):
    """the state digest's sum over a host array of doubles (include/pic1dp_hip.h), as a Python int; no device"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = C.c_uint64()
    check(_lib.load().pic1dp_hip_host_digest(_ptr(a), a.size, C.byref(out)))
    return int(out.value)


def select_thin(fraction):
    """the threshold `thin` of a kept fraction (include/pic1dp_hip.h pic1dp_hip_select_thin): 0 (keep all) for fraction >= 1,
    else max(1, floor(fraction 2^64)); host only"""
    t = C.c_uint64()
    check(_lib.load().pic1dp_hip_select_thin(float(fraction), C.byref(t)))
    return int(t.value)


ZOOM_PLANES = ("markr", "total", "pertb")


def _zoom_planes(which):
    if not 1 <= int(which) <= 7:
        raise Pic1dpError(1, "zoom: which = %d, must be a mask of 1 (markr), 2 (total) and 4 (pertb)" % which)
    return bin(int(which)).count("1")


def _zoom_shape(z):
    """(nvb, nxb), or (0, 0) for a grid the library will refuse (nothing of that size is allocated for the refusal)"""
    ok = 1 <= z.nxb <= 4096 and 1 <= z.nvb <= 4096 and z.nxb * z.nvb <= 2**20
    return (z.nvb, z.nxb) if ok else (0, 0)


def make_zoom(inp, x=None, v=None, bins=(64, 64)):
    """struct pic1dp_zoom from windows (lo, hi) and bins = (nxb, nvb); x=None: the whole box, v=None: [-v_max, v_max)"""
    x = (0.0, inp.lx) if x is None else x
    v = (-inp.v_max, inp.v_max) if v is None else v
    return Zoom(float(x[0]), float(x[1]), float(v[0]), float(v[1]), int(bins[0]), int(bins[1]))


def _split_zoom(out, inp, z, which):
    res = {name: out[j] for j, name in enumerate(n for k, n in enumerate(ZOOM_PLANES) if which & (1 << k))}
    lw = (z.x_hi + inp.lx) - z.x_lo if z.x_lo > z.x_hi else z.x_hi - z.x_lo
    res["x_edges"] = z.x_lo + lw * np.arange(z.nxb + 1) / z.nxb
    res["v_edges"] = z.v_lo + (z.v_hi - z.v_lo) * np.arange(z.nvb + 1) / z.nvb
    return res


def zoom_len(x, v, bins, which=7):
    """doubles pic1dp_hip_zoom hands out for this window, grid and mask: nplanes * nxb * nvb (host only)"""
    z, n = Zoom(float(x[0]), float(x[1]), float(v[0]), float(v[1]), int(bins[0]), int(bins[1])), C.c_int64()
    check(_lib.load().pic1dp_hip_zoom_len(C.byref(z), int(which), C.byref(n)))
    return n.value


def zoom_convert(inp, limbs, x=None, v=None, bins=(64, 64), which=7, ispecies=0):
    """limbs of zoom_local_exact (or their element-wise sum over ranks) -> the dict zoom() returns: every cell's integer
    total converted once (host only, no device)"""
    z = make_zoom(inp, x, v, bins)
    a = np.ascontiguousarray(limbs, dtype=np.int64)
    m = C.c_int64()
    check(_lib.load().pic1dp_hip_zoom_limbs_len(C.byref(z), int(which), C.byref(m)))
    if a.size != m.value:
        raise ValueError("limbs: %d words, %d expected" % (a.size, m.value))
    out = np.zeros((_zoom_planes(which),) + _zoom_shape(z))
    check(_lib.load().pic1dp_hip_zoom_convert(C.byref(inp), int(ispecies), C.byref(z), int(which), _ptr(a), _ptr(out)))
    return _split_zoom(out, inp, z, which)


def host_zoom(inp, xs, vs, ps=None, ws=None, x=None, v=None, bins=(64, 64), which=7, ispecies=0):
    """the zoom's rule and sums on host arrays of valid markers (include/pic1dp_hip.h pic1dp_hip_host_zoom; no device):
    (limbs of shape (nplanes, 2, nvb, nxb), normalised, of the terms summed; rejected[3], the terms not summed per plane)"""
    z = make_zoom(inp, x, v, bins)
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (xs, vs, ps, ws)]
    n = arrs[0].size
    if any(a is not None and a.size != n for a in arrs):
        raise ValueError("the marker arrays must have one length")
    limbs = np.zeros((_zoom_planes(which), 2) + _zoom_shape(z), dtype=np.int64)
    rej = np.zeros(3, dtype=np.int64)
    check(_lib.load().pic1dp_hip_host_zoom(C.byref(inp), int(ispecies), C.byref(z), int(which), *[None if a is None else _ptr(a) for a in arrs],
                                           n, _ptr(limbs), _ptr(rej)))
    return limbs, rej


def make_hermite(modes=(1,), nherm=64, v0=0.0, vt=1.0):
    """struct pic1dp_hermite from the Fourier modes (at most eight), the number of Hermite rows and the scaling
    u = (v - v0) / vt; more than eight modes are left to the library to refuse (nmodes says how many were given)"""
    modes = [int(m) for m in modes]
    h = Hermite(int(nherm), len(modes), (C.c_int32 * 8)(*modes[:8]), float(v0), float(vt))
    return h


def _hermite_shape(h, which):
    """(nsets, nmodes, 2, nherm), or zeros for a shape the library will refuse"""
    nsets = 2 if which == 3 else 1
    ok = 1 <= h.nherm <= 256 and 1 <= h.nmodes and nsets * h.nmodes <= 8
    return (nsets, h.nmodes, 2, h.nherm) if ok else (0, 0, 2, 0)


def _split_hermite(out, which):
    names = [n for bit, n in ((1, "total"), (2, "pertb")) if which & bit]
    return {name: out[j, :, 0, :] - 1j * out[j, :, 1, :] for j, name in enumerate(names)}


def hermite_len(modes=(1,), nherm=64, which=3, v0=0.0, vt=1.0):
    """doubles pic1dp_hip_hermite hands out: nsets * nmodes * 2 * nherm (host only)"""
    h, n = make_hermite(modes, nherm, v0, vt), C.c_int64()
    check(_lib.load().pic1dp_hip_hermite_len(C.byref(h), int(which), C.byref(n)))
    return n.value


def hermite_tables(nherm):
    """(ra, rb) of the recurrence psi_(n+1) = (u psi_n) ra[n] - psi_(n-1) rb[n]: 1 / sqrt(n + 1) and sqrt(n) / sqrt(n + 1)
    as the library rounds them (host only)"""
    ra, rb = np.zeros(max(int(nherm), 0)), np.zeros(max(int(nherm), 0))
    check(_lib.load().pic1dp_hip_hermite_tables(int(nherm), _ptr(ra), _ptr(rb)))
    return ra, rb


def host_hermite(inp, xs, vs, ps=None, ws=None, modes=(1,), nherm=64, v0=0.0, vt=1.0, which=3, ispecies=0):
    """the spectrum's terms on host arrays of valid markers, summed in marker order in doubles (include/pic1dp_hip.h
    pic1dp_hip_host_hermite; no device): the raw sums, shape (nsets, nmodes, 2, nherm), [..., 0, :] cos and [..., 1, :] sin"""
    h = make_hermite(modes, nherm, v0, vt)
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (xs, vs, ps, ws)]
    n = arrs[0].size
    if any(a is not None and a.size != n for a in arrs):
        raise ValueError("the marker arrays must have one length")
    out = np.zeros(_hermite_shape(h, which))
    check(_lib.load().pic1dp_hip_host_hermite(C.byref(inp), int(ispecies), int(which), C.byref(h), n,
                                              *[None if a is None else _ptr(a) for a in arrs], _ptr(out)))
    return out


def hermite_functions(u, nherm):
    """psi_0 .. psi_(nherm-1), the orthonormal probabilists' Hermite polynomials, at every u by the library's recurrence in
    numpy -- the same bits as the device's: shape (nherm,) + u.shape"""
    u = np.asarray(u, dtype=np.float64)
    n1 = np.arange(1, int(nherm) + 1, dtype=np.float64)
    ra, rb = 1.0 / np.sqrt(n1), np.sqrt(n1 - 1.0) / np.sqrt(n1)
    psi = np.empty((int(nherm),) + u.shape)
    prev, cur = np.zeros_like(u), np.ones_like(u)
    for n in range(int(nherm)):
        psi[n] = cur
        nxt = u.copy() if n == 0 else (u * cur) * ra[n] - prev * rb[n]
        prev, cur = cur, nxt
    return psi


def hermite_series(g, v, v0=0.0, vt=1.0):
    """sum_n g[n] psi_n(u) exp(-u^2 / 2) / (sqrt(2 pi) vt) at every v, u = (v - v0) / vt: the velocity profile delta f_k(v)
    a row of Pic1dp.hermite() stands for (g real or complex, last axis n)"""
    g = np.asarray(g)
    u = (np.asarray(v, dtype=np.float64) - v0) * (1.0 / vt)
    psi = hermite_functions(u, g.shape[-1])
    return np.tensordot(g, psi, axes=([-1], [0])) * (np.exp(-0.5 * u * u) / (np.sqrt(2.0 * np.pi) * vt))


def make_select(x=(-np.inf, np.inf), v=(-np.inf, np.inf), fraction=1.0, key=0, origin=0, thin=None):
    """struct pic1dp_select from windows (lo, hi), a kept fraction (or the threshold itself: thin), the hash's key and the
    global index of logical marker 0"""
    return Select(float(x[0]), float(x[1]), float(v[0]), float(v[1]), select_thin(fraction) if thin is None else int(thin),
                  int(key) & (2**64 - 1), int(origin))


def host_select(inp, x, v, x_window=(-np.inf, np.inf), v_window=(-np.inf, np.inf), fraction=1.0, key=0, origin=0, max=None,
                thin=None):
    """the selection rule on host arrays x, v of valid markers (include/pic1dp_hip.h pic1dp_hip_host_select; lx from the
    input; no device): (count, the first min(count, max) logical indices); max=None: all of them"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    v = np.ascontiguousarray(v, dtype=np.float64)
    if x.size != v.size:
        raise ValueError("x and v must have one length")
    sel, n = make_select(x_window, v_window, fraction, key, origin, thin), C.c_int64()
    L = _lib.load()
    if max is None:
        check(L.pic1dp_hip_host_select(C.byref(inp), C.byref(sel), _ptr(x), _ptr(v), x.size, 0, C.byref(n), None))
        max = n.value
    index = np.empty(int(max), dtype=np.int64)
    check(L.pic1dp_hip_host_select(C.byref(inp), C.byref(sel), _ptr(x), _ptr(v), x.size, int(max), C.byref(n), _ptr(index)))
    return n.value, index[:min(n.value, int(max))]


def load_origin(inp, ispecies=0, rank=0, nranks=1, npe=0):
    """global index of the first valid marker of species `ispecies` that the process (rank, nranks, npe) owns under
    particle_load_device: the valid markers of the reference blocks before its first one (host only, no device)"""
    lay, g0 = Layout(rank, nranks, npe, -1), C.c_int64()
    check(_lib.load().pic1dp_hip_load_origin(C.byref(inp), C.byref(lay), int(ispecies), C.byref(g0)))
    return g0.value


def load_uniforms(kind, g0, n, seed_offset=0, ispecies=0):
    """(u_v, u_x) of the global markers g0 ... g0 + n - 1 under particle_load_device(kind), computed on the host"""
    uv, ux = np.empty(int(n)), np.empty(int(n))
    check(_lib.load().pic1dp_hip_host_load_uniforms(int(kind), int(seed_offset), int(ispecies), int(g0), int(n), _ptr(uv), _ptr(ux)))
    return uv, ux


def checkpoint_info(path):
    """what a checkpoint file says about itself (lengths and checksum verified; host only): the input, the layout, the
    seven settings by name, itime, time, counters, sizes and the marker sections' digests"""
    inp, info = Input(), _lib.CheckpointInfo()
    check(_lib.load().pic1dp_hip_checkpoint_info(os.fsencode(path), C.byref(inp), C.byref(info)))
    ns = info.nspecies
    return {"input": inp, "format_version": info.format_version, "file_bytes": info.file_bytes, "input_size": info.input_size,
            "rank": info.layout.rank, "nranks": info.layout.nranks, "npe": info.layout.npe, "nblk": info.nblk,
            "settings": {n: int(info.settings[i]) for i, n in enumerate(Pic1dp.SETTING_NAMES)},
            "itime": info.itime, "time": info.time, "imerge": info.imerge, "iremove": info.iremove, "isplit": info.isplit,
            "rng_ready": bool(info.rng_ready), "hist_count": info.hist_count,
            "nalloc": [int(info.nalloc[s]) for s in range(ns)], "np": [int(info.np[s]) for s in range(ns)],
            "digest": [[int(info.digest[s][k]) for k in range(4)] for s in range(ns)], "checksum": int(info.checksum)}


def checkpoint_verify(path):
    """every checksum and digest of a checkpoint file recomputed on the host; raises Pic1dpError naming what fails"""
    check(_lib.load().pic1dp_hip_checkpoint_verify(os.fsencode(path)))


def field_transform_supported(nx, transform=1):
    """does field transform `transform` handle a grid of nx cells?  (host only, no device)"""
    ok = C.c_int32()
    check(_lib.load().pic1dp_hip_field_transform_supported(int(nx), int(transform), C.byref(ok)))
    return bool(ok.value)


def device_count():
    return _lib.load().pic1dp_hip_device_count()


def tuning_build():
    """True when the loaded library is a -DPIC1DP_TUNING build (it then reads the measurement knobs of tools/README.md)"""
    return _lib.load().pic1dp_hip_tuning_build() == 1
