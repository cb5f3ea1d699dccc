"""ctypes binding of libpic1dp_probe.so (include/pic1dp_probe.h): MEASUREMENT and test support.

Streaming-rate probes with the marker kernels' access shapes (bench.py's second roofline
denominator, tools/) and array evaluations of the device functions the marker kernels call
(the parity tests).  Not imported by the package: the product is libpic1dp_hip.so alone.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PIC1DP_PROBE_LIB") or os.path.join(HERE, "lib", "libpic1dp_probe.so")


class Species(C.Structure):
    """struct pic1dp_probe_species: one species of the input (src/pic1dp_input.F90:43-72)"""
    _fields_ = [("iptcldist", C.c_int32), ("charge", C.c_double), ("mass", C.c_double),
                ("temperature", C.c_double), ("temperature2", C.c_double), ("density", C.c_double),
                ("v0", C.c_double)]


class LaunchQuery(C.Structure):
    """struct pic1dp_probe_launch_query: what the launch policy sees of the context, a kernel family and its arguments"""
    _fields_ = [(n, C.c_int32) for n in ("num_cu", "threads_req", "bpc_req", "osub_req", "family", "nx", "nmode")] + [
        ("np", C.c_int64)] + [(n, C.c_int32) for n in ("full", "exact", "with_E", "with_rho", "priv", "pred_kind",
                                                       "exp_bearing", "nx_opd", "nv_opd")]


STEP_QUERY_SETTINGS = ("fuse_solve", "tail_on", "call_pair", "lazy_calls", "predict", "carry", "osub_req", "dyn_tail", "dyn_tail_full",
                       "pred_kind_req", "gcopies_req", "one_rank_order")
STEP_QUERY_KNOBS = ("charge_sum", "diag_sum", "fuse_output", "step_mode", "field_solver", "field_transform", "comm", "xchg", "field_npe",
                    "chain_mfma", "has_pred")
STEP_QUERY_CALLS = ("full", "diag", "pred", "tail_ok", "eh_modes", "nt_force", "pred_fresh", "tail_done", "into_E", "pending", "have_eh",
                    "steps_left", "output_now", "output_next", "optimize_now", "optimize_next")


class StepQuery(C.Structure):
    """struct pic1dp_probe_step_query: settings, device, knobs, species facts, and the arguments of the three plans"""
    _fields_ = ([(n, C.c_int32) for n in STEP_QUERY_SETTINGS] + [("nt_threshold_half", C.c_double), ("nt_threshold_full", C.c_double)] +
                [(n, C.c_int32) for n in ("num_cu", "threads_req", "bpc_req") + STEP_QUERY_KNOBS] +
                [("pow2", C.c_int32 * 8), ("one_exp", C.c_int32 * 8), ("np", C.c_int64 * 8)] + [(n, C.c_int32) for n in STEP_QUERY_CALLS])


_D = C.POINTER(C.c_double)
_I64 = C.POINTER(C.c_int64)
_I32 = C.POINTER(C.c_int32)
_SP = C.POINTER(Species)
SIGNATURES = {
    "pic1dp_probe_last_error": [],
    "pic1dp_probe_stream": [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _D],
    "pic1dp_probe_layout": [C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _D],
    "pic1dp_probe_sweep": [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _D],
    "pic1dp_probe_release": [],
    "pic1dp_probe_div_lx": [C.c_int32, C.c_double, C.c_int32, C.c_int64, C.c_uint64, _I64],
    "pic1dp_probe_host_div_lx": [C.c_double, C.c_int32, C.c_int64, C.c_uint64, _I64],
    "pic1dp_probe_div_const": [C.c_int32, C.c_double, C.c_int64, C.c_uint64, _I64],
    "pic1dp_probe_host_div_const": [C.c_double, C.c_int64, C.c_uint64, _I64],
    "pic1dp_probe_diag_div": [C.c_int32, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_int64, C.c_uint64, _I64],
    "pic1dp_probe_host_diag_div": [C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_int64, C.c_uint64, _I64],
    "pic1dp_probe_host_optimize": [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_uint64, C.c_int64,
                                   C.c_int64, _I64, _I64],
    "pic1dp_probe_locate": [C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, _I32],
    "pic1dp_probe_exp": [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64],
    "pic1dp_probe_fx_raise": [C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, _D],
    "pic1dp_probe_species_const": [_SP, _I32, _I32, _I32, _I32, _D],
    "pic1dp_probe_dlnf0": [C.c_int32, _SP, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64],
    "pic1dp_probe_host_launch_shape": [C.POINTER(LaunchQuery), _I64],
    "pic1dp_probe_host_field_lds": [C.c_int32] * 7 + [_I64],
    "pic1dp_probe_host_diag_launch": [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _I64],
    "pic1dp_probe_host_moments_plan": [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _I64],
    "pic1dp_probe_host_moments_plan_exact": [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _I64],
    "pic1dp_probe_host_power_plan": [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _I64],
    "pic1dp_probe_host_power_plan_exact": [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _I64],
    "pic1dp_probe_host_select_plan": [C.c_int64, C.c_int32, C.c_int32, C.c_int32, _I64],
    "pic1dp_probe_host_hermite_plan": [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _I64],
    "pic1dp_probe_hermite": [_D, C.c_int64, C.c_int32, _D],
    "pic1dp_probe_host_zoom_plan": [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _I64],
    "pic1dp_probe_host_dist_scale": [C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32, _I32],
    "pic1dp_probe_host_context_plan": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _I64, C.c_int64, _D],
    "pic1dp_probe_host_settings": [_I32, _D],
    "pic1dp_probe_host_step_plan": [C.c_void_p, C.c_void_p, C.POINTER(StepQuery), _I64, C.c_void_p],
    "pic1dp_probe_host_call_plan": [_I32, _I32, _I32, C.c_int32, _I32],
    "pic1dp_probe_host_load_launch": [C.c_int64, C.c_int32, _I64],
    "pic1dp_probe_host_plain_chunks": [C.c_int64, C.c_int64, C.c_int32, _I64],
    "pic1dp_probe_host_block_layout": [_I64, _I64, C.c_int32, _I64, _I64],
    "pic1dp_probe_write_stream": [C.c_int32, C.c_int64, C.c_int32, _D],
    "pic1dp_probe_load_uniforms": [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
}
PLAN_FIELDS = ("npe", "nblk", "blk0", "nalloc", "imerge", "iremove", "isplit", "gcopies", "gstride", "rho_set_doubles", "pred_kind",
               "pred_private", "pred_set_doubles", "pack_doubles", "tab_lds", "field_npe")
SETTINGS_INTS = ("fuse_solve", "tail_on", "call_pair", "lazy_calls", "predict", "carry", "osub_req", "dyn_tail", "dyn_tail_full",
                 "diag_fx", "pred_kind_req", "chain_mfma_req", "gcopies_req", "field_one_rank_order", "chain_selftest_verbose")
SETTINGS_DOUBLES = ("nt_threshold_half", "nt_threshold_full", "diag_fx_margin_w")

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libpic1dp_probe.so not found at %s -- build it with `python pic1dp_amd/build.py`" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_char_p if name == "pic1dp_probe_last_error" else C.c_int
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise RuntimeError("pic1dp_probe: %s" % (load().pic1dp_probe_last_error() or b"").decode())


def species(inp, isp=0):
    """the probe's species struct from an input object (field names of src/pic1dp_input.F90)"""
    return Species(inp.iptcldist, inp.species_charge[isp], inp.species_mass[isp], inp.species_temperature[isp],
                   inp.species_temperature2[isp], inp.species_density[isp], inp.species_v0[isp])


def stream(nread, nwrite, n, reps=10, device=0, blocks=0, threads=0, variant=None):
    """GB/s of a pure streaming pass: nread arrays of n doubles read, nwrite written (non-temporal by default;
    PIC1DP_PROBE_VARIANT: 0 plain, 2 plain with two pairs per lane)"""
    if variant is None:
        variant = int(os.environ.get("PIC1DP_PROBE_VARIANT", "1"))
    g = C.c_double()
    _check(load().pic1dp_probe_stream(device, nread, nwrite, int(n), reps, blocks, threads, variant, C.byref(g)))
    return g.value


def layout(n, log2_tile=12, reps=10, device=0, stagger_bytes=0, keep=0, blocks=0, threads=0):
    """ms per launch of the second sub-step kernel's traffic (4 arrays read, 3 written back in place) over a fresh
    slab: [arrays apart r/w, tiled r/w, arrays apart read-only, tiled read-only, tiled r/w one workgroup per tile,
    the same read-only]"""
    ms = (C.c_double * 6)()
    _check(load().pic1dp_probe_layout(device, int(n), log2_tile, int(stagger_bytes), reps, keep, blocks, threads, ms))
    return list(ms)


def sweep(n, alternate, plain_bytes=0, pairs=10, trials=5, head_only=False, log2_tile=12, device=0, blocks=0, threads=0):
    """ms per launch, one figure per trial, of launch pairs of the tiled 4-read / 3-write traffic back to back over one
    slab of n markers: alternate 0 forward -> forward, 1 forward -> backward (mirrored 64-pair chunks).  plain_bytes of
    marker state at either slab end (head_only: at the head alone) use plain accesses, the rest non-temporal ones (0: none,
    < 0: all plain)"""
    ms = (C.c_double * trials)()
    _check(load().pic1dp_probe_sweep(device, int(n), log2_tile, int(alternate), int(plain_bytes), int(bool(head_only)), pairs, trials, blocks,
                                     threads, ms))
    return list(ms)


def release():
    _check(load().pic1dp_probe_release())


def div_lx_mismatches(lx, nx, n, seed, device=0, host=False):
    m = C.c_int64(-1)
    L = load()
    if host:
        _check(L.pic1dp_probe_host_div_lx(lx, nx, n, seed, C.byref(m)))
    else:
        _check(L.pic1dp_probe_div_lx(device, lx, nx, n, seed, C.byref(m)))
    return m.value


def diag_div_mismatches(lx, nxo, vmax, nvo, n, seed, device=0, host=False):
    m = C.c_int64(-1)
    L = load()
    if host:
        _check(L.pic1dp_probe_host_diag_div(lx, nxo, vmax, nvo, n, seed, C.byref(m)))
    else:
        _check(L.pic1dp_probe_diag_div(device, lx, nxo, vmax, nvo, n, seed, C.byref(m)))
    return m.value


def div_const_mismatches(divisor, n, seed, device=0, host=False):
    m = C.c_int64(-1)
    L = load()
    if host:
        _check(L.pic1dp_probe_host_div_const(divisor, n, seed, C.byref(m)))
    else:
        _check(L.pic1dp_probe_div_const(device, divisor, n, seed, C.byref(m)))
    return m.value


def locate(x, lx, nx, form, device=0):
    """(ix, wl, two_ops): the marker kernels' locate on the positions x (at most 2^20); form 0 divides by lx in five
    operations, form 1 in two where the host proves them for lx (two_ops tells)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    ix = np.empty(x.size, dtype=np.int32)
    wl = np.empty(x.size, dtype=np.float64)
    two = C.c_int32(-1)
    _check(load().pic1dp_probe_locate(device, float(lx), int(nx), int(form), x.ctypes.data_as(C.c_void_p),
                                      ix.ctypes.data_as(C.c_void_p), wl.ctypes.data_as(C.c_void_p), x.size, C.byref(two)))
    return ix, wl, two.value


def device_exp(x, device=0):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    _check(load().pic1dp_probe_exp(device, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), x.size))
    return y


def fx_raise(bound0, events, device=0):
    """the prediction tiles' fixed-point bound after the raises of workgroups that finish in the given order: events is a
    list of (noted code, start bound) -- code 0 no marker met, 1 none within the bound, 2 + the bits of the float32 value
    met otherwise (fx_code); start: the bound the workgroup started with (device_fx.hpp fx_raise)"""
    noted = np.ascontiguousarray([int(e[0]) for e in events], dtype=np.uint32)
    start = np.ascontiguousarray([float(e[1]) for e in events], dtype=np.float64)
    out = C.c_double()
    _check(load().pic1dp_probe_fx_raise(device, float(bound0), noted.ctypes.data, start.ctypes.data, len(events), C.byref(out)))
    return out.value


def fx_code(value):
    """the code a workgroup notes for the largest value it met within the bound (kernels_step.hip fx_note)"""
    return int(np.float32(value).view(np.uint32)) + 2


def species_const(sp):
    """dict(pow2, unit, fastc, one_exp, f=[fq2, fq1, fq0, fm1, fm0, fd1, fd0]) as the library would form them"""
    a, b, c_, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    f = (C.c_double * 7)()
    _check(load().pic1dp_probe_species_const(C.byref(sp), C.byref(a), C.byref(b), C.byref(c_), C.byref(d), f))
    return dict(pow2=a.value, unit=b.value, fastc=c_.value, one_exp=d.value, f=list(f))


def dlnf0(sp, v, form, device=0):
    """-f0'/f0 at v as the marker kernels evaluate it: form 0 reference operation order, 1 one-exp form"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    y = np.empty_like(v)
    _check(load().pic1dp_probe_dlnf0(device, C.byref(sp), form, v.ctypes.data_as(C.c_void_p),
                                     y.ctypes.data_as(C.c_void_p), v.size))
    return y


def host_optimize_mismatches(kind, np_, nalloc, threshold, seed=1, typeremove=2, nx=32, nv=64, split_ngroup=3):
    """the key-walking planners of the GPU marker optimisation against the host routines on whole markers (0 merge, 1
    remove, 2 split), on the host: (slots that differ (-1 / -2: marker counts / random stream differ), markers after the event)"""
    m, after = C.c_int64(), C.c_int64()
    _check(load().pic1dp_probe_host_optimize(kind, typeremove, nx, nv, split_ngroup, threshold, seed, int(np_), int(nalloc),
                                             C.byref(m), C.byref(after)))
    return m.value, after.value


def host_launch_shape(**query):
    """(threads, blocks, LDS bytes, resident workgroups) the library's launch policy picks (csrc/launch_policy.hpp), on the
    host; keywords: the fields of LaunchQuery (the others 0)"""
    out = (C.c_int64 * 4)()
    if load().pic1dp_probe_host_launch_shape(C.byref(LaunchQuery(**query)), out) != 0:
        raise ValueError("pic1dp_probe_host_launch_shape: unknown family %r" % (query.get("family"),))
    return tuple(out)


def host_field_lds(family, nx, nmode=1, npe=1, tab_lds=1, with_xchg=0, pred_kind=1):
    """(dynamic LDS bytes, threads, kernel) of a one-workgroup field launch (csrc/field_lds.hpp), on the host; family 0 the
    plain solves, 1 launch_field_solve_pair; kernel: 0 k_field_solve..., 1 k_field_solve_pair, 2 _pair1, 3 _pair_sums1"""
    out = (C.c_int64 * 3)()
    if load().pic1dp_probe_host_field_lds(family, nx, nmode, npe, tab_lds, with_xchg, pred_kind, out) != 0:
        raise ValueError("pic1dp_probe_host_field_lds: unknown family %r" % (family,))
    return tuple(out)


def host_diag_launch(kind, np_, nx_opd, nv_opd, num_cu, ntail=0):
    """(blocks, threads, LDS copy or not, dynamic LDS bytes, NT, tail-slot workgroups) of a diagnostics pass of output_all
    (csrc/launch_policy.hpp diag_launch), on the host; kind 0 k_ptcldist, 1 k_ptcldist_exact"""
    out = (C.c_int64 * 6)()
    if load().pic1dp_probe_host_diag_launch(kind, int(np_), nx_opd, nv_opd, num_cu, int(ntail), out) != 0:
        raise ValueError("pic1dp_probe_host_diag_launch: unknown kind %r" % (kind,))
    return tuple(out)


MOMENTS_PASS_FIELDS = ("blocks", "threads", "nt", "bytes", "sets", "kmask", "first_plane", "planes")
POWER_PASS_FIELDS = ("blocks", "threads", "nt", "bytes", "sets", "lds", "first_set", "nsets")


def host_power_plan(nx, nx_opd, nv_opd, which, deltaf, np_, num_cu):
    """the passes of one power call (csrc/launch_policy.hpp power_plan), on the host: dict(selected, tile, plane, passes) with
    one dict of POWER_PASS_FIELDS per pass (sets: bit 0 p, bit 1 w; lds: the planes in the workgroup's LDS, 0: straight in
    memory); no pass: an unknown `which`, w asked of a full-f run, a grid out of range"""
    out = (C.c_int64 * 20)()
    if load().pic1dp_probe_host_power_plan(int(nx), int(nx_opd), int(nv_opd), int(which), int(deltaf), int(np_), int(num_cu), out) != 0:
        raise ValueError("pic1dp_probe_host_power_plan")
    return dict(selected=out[1], tile=out[2], plane=out[3],
                passes=[dict(zip(POWER_PASS_FIELDS, out[4 + 8 * i:12 + 8 * i])) for i in range(out[0])])


def host_power_plan_exact(nx, nx_opd, nv_opd, which, deltaf, np_, num_cu):
    """the passes of one power_exact call (csrc/launch_policy.hpp power_plan_exact), as host_power_plan returns them: the
    same passes, bytes, NT and sets; blocks = max(1, min(num_cu, ceil(np / 2^17)))"""
    out = (C.c_int64 * 20)()
    if load().pic1dp_probe_host_power_plan_exact(int(nx), int(nx_opd), int(nv_opd), int(which), int(deltaf), int(np_), int(num_cu), out) != 0:
        raise ValueError("pic1dp_probe_host_power_plan_exact")
    return dict(selected=out[1], tile=out[2], plane=out[3],
                passes=[dict(zip(POWER_PASS_FIELDS, out[4 + 8 * i:12 + 8 * i])) for i in range(out[0])])


ZOOM_PASS_FIELDS = ("blocks", "threads", "nt", "bytes", "planes", "lds", "first_row", "rows")


def host_zoom_plan(nxb, nvb, which, deltaf, np_, num_cu, pass_cap=0):
    """the passes of one zoom call (csrc/launch_policy.hpp zoom_plan), on the host: dict(selected, pass_cap, passes) with one
    dict of ZOOM_PASS_FIELDS per pass (planes: bit 0 markr, 1 total, 2 pertb; lds: the band's words in the workgroup's LDS,
    0: every row straight in memory); pass_cap=0: the library's; no pass: arguments out of range"""
    out = (C.c_int64 * 515)()
    if load().pic1dp_probe_host_zoom_plan(int(nxb), int(nvb), int(which), int(deltaf), int(np_), int(num_cu), int(pass_cap), out) != 0:
        raise ValueError("pic1dp_probe_host_zoom_plan")
    return dict(selected=out[1], pass_cap=out[2], passes=[dict(zip(ZOOM_PASS_FIELDS, out[3 + 8 * i:11 + 8 * i])) for i in range(out[0])])


HERMITE_PLAN_FIELDS = ("blocks", "threads", "nt", "bytes", "nb", "partials")


def host_hermite_plan(nherm, nmodes, which, deltaf, np_, num_cu):
    """the pass of one hermite call (csrc/launch_policy.hpp hermite_plan), on the host: a dict of HERMITE_PLAN_FIELDS
    (partials: the partial sums merged into one output word -- B of the error bound); blocks 0: arguments out of range"""
    out = (C.c_int64 * 6)()
    if load().pic1dp_probe_host_hermite_plan(int(nherm), int(nmodes), int(which), int(deltaf), int(np_), int(num_cu), out) != 0:
        raise ValueError("pic1dp_probe_host_hermite_plan")
    return dict(zip(HERMITE_PLAN_FIELDS, out[:]))


def hermite(u, nherm):
    """psi_0 .. psi_(nherm-1) at every u by the DEVICE's recurrence (csrc/device_hermite.hpp), shape (len(u), nherm)"""
    u = np.ascontiguousarray(u, dtype=np.float64)
    out = np.zeros((u.size, int(nherm)))
    _check(load().pic1dp_probe_hermite(u.ctypes.data_as(_D), u.size, int(nherm), out.ctypes.data_as(_D)))
    return out


SELECT_PLAN_FIELDS = ("chunk_pairs", "nchunk", "blocks", "threads", "nt", "scan_threads")


def host_select_plan(np_, num_cu, threads=0, blocks_per_cu=0):
    """the count and write passes of a selection over np_ valid markers (csrc/launch_policy.hpp select_plan), on the host: a
    dict of SELECT_PLAN_FIELDS.  Chunk c holds the logical pairs [c chunk_pairs, min((c + 1) chunk_pairs, np_ // 2)), the
    odd last marker belongs to the last chunk"""
    out = (C.c_int64 * 6)()
    if load().pic1dp_probe_host_select_plan(int(np_), int(num_cu), int(threads), int(blocks_per_cu), out) != 0:
        raise ValueError("pic1dp_probe_host_select_plan")
    return dict(zip(SELECT_PLAN_FIELDS, out[:]))


def host_moments_plan(nx, which, deltaf, np_, num_cu):
    """the passes of one moments call (csrc/launch_policy.hpp moments_plan), on the host: dict(selected, group, passes) with
    one dict of MOMENTS_PASS_FIELDS per pass (sets: bit 0 p, bit 1 w; kmask: bit k = v^k); no pass: an unknown `which`, w
    asked of a full-f run, nx out of range"""
    out = (C.c_int64 * 35)()
    if load().pic1dp_probe_host_moments_plan(int(nx), int(which), int(deltaf), int(np_), int(num_cu), out) != 0:
        raise ValueError("pic1dp_probe_host_moments_plan")
    return dict(selected=out[1], group=out[2],
                passes=[dict(zip(MOMENTS_PASS_FIELDS, out[3 + 8 * i:11 + 8 * i])) for i in range(out[0])])


def host_moments_plan_exact(nx, which, deltaf, np_, num_cu):
    """the passes of one moments_exact call (csrc/launch_policy.hpp moments_plan_exact), as host_moments_plan returns them:
    the same groups, bytes, NT, sets and powers; blocks = max(1, min(num_cu, ceil(np / 2^17)))"""
    out = (C.c_int64 * 35)()
    if load().pic1dp_probe_host_moments_plan_exact(int(nx), int(which), int(deltaf), int(np_), int(num_cu), out) != 0:
        raise ValueError("pic1dp_probe_host_moments_plan_exact")
    return dict(selected=out[1], group=out[2],
                passes=[dict(zip(MOMENTS_PASS_FIELDS, out[3 + 8 * i:11 + 8 * i])) for i in range(out[0])])


def host_dist_scale(np_, blocks, deltaf, bound_p, bound_w, threads=1024):
    """(fixed point or not, log2 scale of markr, total, pertb) a fixed-point diagnostics pass would use
    (csrc/kernels.hpp make_dist_scale), on the host"""
    out = (C.c_int32 * 4)()
    if load().pic1dp_probe_host_dist_scale(int(np_), blocks, deltaf, bound_p, bound_w, threads, out) != 0:
        raise ValueError("pic1dp_probe_host_dist_scale")
    return tuple(out)


def host_context_plan(inp, nranks=1, npe=0, rank=0, pred_kind_req=0, gcopies_req=0, one_rank_order=0):
    """what pic1dp_hip_create would decide before its first allocation (csrc/context_plan.hpp plan_context), on the host, as
    a dict: PLAN_FIELDS, np [nspecies], blk_alloc [nblk], blk_np [nspecies][nblk], sc_re, sc_im; inp: a pic1dp_amd Input"""
    from ._lib import Layout
    lay = Layout(rank, nranks, npe, -1)
    ns, nblk = inp.nspecies, (npe if npe > 0 else nranks) // nranks
    cap = len(PLAN_FIELDS) + ns + nblk * (1 + ns)
    out, sc = (C.c_int64 * cap)(), (C.c_double * 2)()
    if load().pic1dp_probe_host_context_plan(C.addressof(inp), C.addressof(lay), pred_kind_req, gcopies_req, one_rank_order,
                                             out, cap, sc) != 0:
        raise ValueError("pic1dp_probe_host_context_plan: bad argument")
    v = list(out)
    plan = dict(zip(PLAN_FIELDS, v))
    k = len(PLAN_FIELDS)
    plan["np"] = v[k:k + ns]
    plan["blk_alloc"] = v[k + ns:k + ns + nblk]
    plan["blk_np"] = [v[k + ns + nblk * (1 + s):k + ns + nblk * (2 + s)] for s in range(ns)]
    plan["sc_re"], plan["sc_im"] = sc[0], sc[1]
    return plan


def host_settings():
    """the settings a context created now would take from the environment (csrc/settings.hpp), as a dict"""
    iv, dv = (C.c_int32 * len(SETTINGS_INTS))(), (C.c_double * len(SETTINGS_DOUBLES))()
    if load().pic1dp_probe_host_settings(iv, dv) != 0:
        raise ValueError("pic1dp_probe_host_settings")
    return dict(list(zip(SETTINGS_INTS, iv)) + list(zip(SETTINGS_DOUBLES, dv)))


STEP_CAPS = ("dft_paths", "six_sums_one_mode", "modes_fit_field_kernel", "exp_bearing", "step_recompute_ok", "predict_capable",
             "diag_in_step", "priv", "fuse_capable", "lazy_calls_ok", "pair_serves_collect", "pair_in_solve_field", "pred_kind")
STEP_MARKERS = ("pred", "priv", "diag", "tail_mode", "tail_species", "stream_nt", "solve_species", "solve_fits", "solve_threads", "tag",
                "rd", "wr")
STEP_SPECIES = ("launched", "family", "threads", "blocks", "lds", "dyn_tail", "plain_chunks", "carry", "tail")
STEP_SOLVE = ("refused", "reduce_first", "pack_reduce", "pack_first", "launch", "with_local")
STEP_WHOLE = ("substeps", "finish_pending", "diag", "pred", "fused_in", "adopt_eh", "half_pass", "half_eh_modes", "fuse_out")
STEP_QUERY_DEFAULTS = dict(fuse_solve=1, tail_on=1, call_pair=1, lazy_calls=1, predict=1, carry=-1, dyn_tail=8, dyn_tail_full=16,
                           num_cu=256, has_pred=-1, nt_force=-1, full=1, into_E=1, steps_left=1)


def host_step_plan(inp, nranks=1, npe=0, rank=0, np_=None, pow2=None, one_exp=None, **query):
    """what a time step would launch (csrc/step_plan.hpp), on the host: dict(caps, markers -- with one dict per species
    under "species", name included --, solve, whole) of integers.  query: the fields of StepQuery (the settings at their
    defaults, 256 CUs, a full step into field_electric, the last step of its call unless given); np_ / pow2 / one_exp: per
    species (the plan's marker counts, 0, 0)"""
    from ._lib import Layout
    lay = Layout(rank, nranks, npe, -1)
    q = StepQuery(**dict(STEP_QUERY_DEFAULTS, **query))
    for s in range(8):
        q.np[s] = -1 if np_ is None or s >= len(np_) else int(np_[s])
        q.pow2[s] = 0 if pow2 is None or s >= len(pow2) else int(pow2[s])
        q.one_exp[s] = 0 if one_exp is None or s >= len(one_exp) else int(one_exp[s])
    out, names = (C.c_int64 * 112)(), ((C.c_char * 64) * 8)()
    if load().pic1dp_probe_host_step_plan(C.addressof(inp), C.addressof(lay), C.byref(q), out, C.addressof(names)) != 0:
        raise ValueError("pic1dp_probe_host_step_plan: bad argument")
    v = list(out)
    caps, markers = dict(zip(STEP_CAPS, v[:13])), dict(zip(STEP_MARKERS, v[13:25]))
    markers["species"] = [dict(zip(STEP_SPECIES, v[25 + 9 * s:34 + 9 * s]), name=names[s].value.decode()) for s in range(inp.nspecies)]
    return dict(caps=caps, markers=markers, solve=dict(zip(STEP_SOLVE, v[97:103])), whole=dict(zip(STEP_WHOLE, v[103:112])))


CALL_STATE = ("seq", "owed", "e_step_start", "cd_kept_mode_only", "adopt_current", "charge_pending", "charge_pending_pred", "call_phase",
              "eh_modes")
CALL_MOMENT = ("lazy_calls", "call_pair", "loaded", "several_ranks", "fp64_rank_sum", "charge_sum", "pred_kind", "tab_lds",
               "field_differs", "pred_usable", "eh_current", "modes_current", "optimize_due_any", "output_follows")
CALL_CAPS = ("dft_paths", "six_sums_one_mode", "modes_fit_field_kernel", "predict_capable", "diag_in_step", "lazy_calls_ok",
             "pair_serves_collect", "pair_in_solve_field")
CALL_MOMENT_DEFAULTS = dict(lazy_calls=1, call_pair=1, loaded=1)


# call_plan.hpp enum Call and enum Act, in order
CALL_KINDS = ("push1", "push2", "collect_charge", "charge_local", "charge_reduced", "charge_local_exact", "charge_exact_handed_out",
              "charge_reduced_exact", "solve_field", "markers", "read_markers", "whole_steps", "substep1", "substep2", "read_field",
              "get_field", "get_field_cd", "output_all", "output_all_cd", "write_electric", "write_chargeden", "replace_markers",
              "upload_markers", "switch_field", "between_steps", "checkpoint")
CALL_ACTS = ("save_step_start_field", "adopt_half_field", "adopt_half_modes", "copy_eh_to_e", "push_eager_1", "push_eager_1_from_e0",
             "push_eager_2", "wrap_only", "deposit", "half_pass", "swap_eh", "full_pass", "fx_settle", "reduce_charge", "chargeden",
             "chargeden_sum", "pred_chargeden", "pred_chargeden_summed", "pred_combine", "pred_to_charge", "pred_reduce", "charge_local",
             "fx_to_rho", "solve_pair", "solve_pred_tiles", "solve_pred_sums", "solve_plain", "state_version", "cd_version",
             "field_written_by_solve", "call_pair_skip", "pred_consumed", "mark_eh_current", "span_collect", "span_field", "span_end")


def host_call_plan(call, state=None, moment=None, caps=None):
    """what a call of the call sites' state machine enqueues and which state follows (csrc/call_plan.hpp plan_call), on the
    host: dict(refusal, refused_after, bad=(seq, owed), next=the state that follows, acts=[(name, argument)],
    invariants_hold).  call: its name (CALL_KINDS) or index; state / moment / caps: dicts of the fields of CALL_STATE /
    CALL_MOMENT / CALL_CAPS that are not 0 (moment: lazy call sites with the pair, markers loaded unless given)"""
    calls, acts = CALL_KINDS, CALL_ACTS
    idx = calls.index(call) if isinstance(call, str) else int(call)
    moment = dict(CALL_MOMENT_DEFAULTS, **(moment or {}))
    for given, known in ((state or {}, CALL_STATE), (moment, CALL_MOMENT), (caps or {}, CALL_CAPS)):
        if set(given) - set(known):
            raise ValueError("unknown fields %r" % sorted(set(given) - set(known)))
    st = (C.c_int32 * 9)(*[int((state or {}).get(n, 0)) for n in CALL_STATE])
    mo = (C.c_int32 * 14)(*[int(moment.get(n, 0)) for n in CALL_MOMENT])
    ca = (C.c_int32 * 8)(*[int((caps or {}).get(n, 0)) for n in CALL_CAPS])
    out = (C.c_int32 * 64)()
    if load().pic1dp_probe_host_call_plan(st, mo, ca, idx, out) != 0:
        raise ValueError("pic1dp_probe_host_call_plan: no such kind of call")
    v = list(out)
    return dict(refusal=v[0], refused_after=v[1], bad=(v[2], v[3]), next=dict(zip(CALL_STATE, v[4:13])),
                acts=[(acts[v[14 + 2 * i]], v[15 + 2 * i]) for i in range(v[13])], invariants_hold=v[63])


def host_load_launch(nalloc, num_cu=256):
    """launch shape of the on-device particle load's pass: {blocks, threads, nt, chunk} (host arithmetic, no GPU)"""
    out = (C.c_int64 * 4)()
    if load().pic1dp_probe_host_load_launch(int(nalloc), num_cu, out) != 0:
        raise RuntimeError("pic1dp_probe_host_load_launch: bad argument")
    return dict(blocks=out[0], threads=out[1], nt=bool(out[2]), chunk=out[3])


def host_plain_chunks(np_all_species, np_species, nt=True):
    """the 64-pair chunks at the head of a species' slab that a non-temporal one-pass launch keeps in the Infinity Cache
    with plain accesses (csrc/launch_policy.hpp stream_plain_chunks), on the host"""
    out = C.c_int64(-1)
    if load().pic1dp_probe_host_plain_chunks(int(np_all_species), int(np_species), int(bool(nt)), C.byref(out)) != 0:
        raise ValueError("pic1dp_probe_host_plain_chunks: bad argument")
    return out.value


def host_block_layout(blk_alloc, blk_np):
    """where the blocks of one species lie in its packed arrays (csrc/block_layout.hpp), on the host:
    ([(voff, np, toff, ntail) per block], the species' valid markers)"""
    n = len(blk_alloc)
    out, total = (C.c_int64 * (4 * n))(), C.c_int64(-1)
    if len(blk_np) != n or load().pic1dp_probe_host_block_layout((C.c_int64 * n)(*blk_alloc), (C.c_int64 * n)(*blk_np), n, out,
                                                                 C.byref(total)) != 0:
        raise ValueError("pic1dp_probe_host_block_layout: bad argument")
    return [tuple(out[4 * b:4 * b + 4]) for b in range(n)], total.value


def load_uniforms(kind, g, seed_offset=0, ispecies=0, device=0):
    """(u_v, u_x) of the global marker indices g as the load KERNEL's index function forms them (on the GPU)"""
    g = np.ascontiguousarray(g, dtype=np.int64)
    uv, ux = np.empty(g.size), np.empty(g.size)
    _check(load().pic1dp_probe_load_uniforms(device, kind, seed_offset, ispecies, g.ctypes.data, g.size, uv.ctypes.data,
                                             ux.ctypes.data))
    return uv, ux


def write_stream(n, reps=10, device=0):
    """GB/s of the load kernel's stores without its arithmetic: the four arrays of a tiled slab of n slots written"""
    g = C.c_double()
    _check(load().pic1dp_probe_write_stream(device, int(n), reps, C.byref(g)))
    return g.value
