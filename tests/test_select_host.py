"""Select and gather markers (include/pic1dp_hip.h pic1dp_hip_select) on the host: no GPU.  The
declarations through every layer, the thinning threshold, the library's host form of the rule (pic1dp_hip_host_select)
against tests/select_reference.py bit for bit, the hash's statistics and why thinning is not a stride, the chunk plan of the
kernels through the probe library, and tests/select_check.cpp under the host sanitizers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import select_reference as R
from conftest import ROOT

ERR_ARG = 1
ENTRY_POINTS = ("select_count", "select", "gather", "host_select", "select_thin")


# ---------------------------------------------------------------------------
# declarations
# ---------------------------------------------------------------------------
def test_entry_points_are_declared_in_every_layer(amd):
    lib = C.CDLL(amd._lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pic1dp_hip.h")).read()
    fortran = open(os.path.join(ROOT, "pic1dp_amd", "fortran", "pic1dp_hip_mod.F90")).read()
    for name in ENTRY_POINTS:
        full = "pic1dp_hip_" + name
        assert hasattr(lib, full), name
        assert full in amd._lib.SIGNATURES, name
        assert "int %s(" % full in header, name
        assert 'bind(C, name="%s")' % full in fortran, name
    assert "typedef struct pic1dp_select {" in header and "type, bind(C) :: pic1dp_select_t" in fortran
    assert C.sizeof(amd.Select) == 56
    assert [f[0] for f in amd.Select._fields_] == ["x_lo", "x_hi", "v_lo", "v_hi", "thin", "key", "origin"]
    for f in ("select", "select_count", "gather"):
        assert callable(getattr(amd.Pic1dp, f))
    assert callable(amd.host_select) and callable(amd.select_thin)


def test_header_carries_the_rule_and_the_kernel_stats():
    header = " ".join(open(os.path.join(ROOT, "include", "pic1dp_hip.h")).read().split())
    for line in ("px = wrap(x)",
                 "in_x = x_lo <= px && px < x_hi",
                 "in_x = px >= x_lo || px < x_hi",
                 "in_v = v_lo <= v && v < v_hi",
                 "h(g) = mix64(key + (g + 1) * 0x9E3779B97F4A7C15) mod 2^64, g = origin + i",
                 "selected = in_x && in_v && (thin == 0 || h(g) < thin)",
                 "A NaN bound is PIC1DP_ERR_ARG",
                 "Tail slots (i >= np) are never selected",
                 "thin = max(1, floor(fraction 2^64))",
                 "0 <= index < nalloc",
                 "which = 21:", "which = 22:", "Cost:"):
        assert line in header, line


# ---------------------------------------------------------------------------
# select_thin
# ---------------------------------------------------------------------------
def test_select_thin(amd):
    assert amd.select_thin(1.0) == 0 and amd.select_thin(2.0) == 0 and amd.select_thin(math.inf) == 0
    assert amd.select_thin(0.5) == 2**63
    assert amd.select_thin(2.0**-64) == 1
    assert amd.select_thin(2.0**-70) == 1                    # max(1, 0)
    assert amd.select_thin(1.0 - 2.0**-53) == 2**64 - 2**11
    assert amd.select_thin(1.0 / 16.0) == 2**60
    for f in (1.0 / 3.0, 0.1, 1e-9, 0.75, 2.0**-64 * 1.5, math.nextafter(1.0, 0.0), 5e-324):
        assert amd.select_thin(f) == R.thin_of(f), f
    for bad in (0.0, -0.0, -1.0, math.nan, -math.inf):
        with pytest.raises(amd.Pic1dpError) as ei:
            amd.select_thin(bad)
        assert ei.value.code == ERR_ARG and "fraction" in str(ei.value)
    assert amd._lib.load().pic1dp_hip_select_thin(0.5, None) == ERR_ARG


# ---------------------------------------------------------------------------
# host_select against the reference
# ---------------------------------------------------------------------------
V_LO, V_HI = -1.5, 2.25


@pytest.fixture(scope="module")
def crafted(amd):
    inp = amd.make_input(nparticle_max=16, nx=16)
    x, v, p, w = R.edge_markers(inp.lx, V_LO, V_HI)
    return inp, dict(x=x, v=v, p=p, w=w)


def test_crafted_markers_hold_every_edge(crafted):
    inp, g = crafted
    px = R.wrapped(g["x"], inp.lx)
    assert np.any(px == inp.lx)                              # -1e-300 + lx rounds to lx: used as it is
    assert np.any(np.signbit(g["x"]) & (g["x"] == 0.0)) and np.any(np.isnan(px)) and np.any(np.isinf(g["v"]))
    assert g["x"].size == 9 * 7 + 300


@pytest.mark.parametrize("thin", [0, 2**62], ids=["all", "quarter"])
def test_host_select_equals_the_reference_on_crafted_markers(amd, crafted, thin):
    inp, g = crafted
    seen = {}
    for name, xw, vw in R.windows(inp.lx, V_LO, V_HI):
        ref = R.select(g, inp.lx, x_window=xw, v_window=vw, thin=thin, key=3)
        count, index = amd.host_select(inp, g["x"], g["v"], xw, vw, thin=thin, key=3)
        assert count == ref["count"] and np.array_equal(index, ref["index"]), name
        seen[name] = count
        print("host_select %s thin %d: %d of %d" % (name, thin, count, g["x"].size))
        for m in sorted({0, 1, max(count - 1, 0), count, count + 1}):
            c2, i2 = amd.host_select(inp, g["x"], g["v"], xw, vw, thin=thin, key=3, max=m)
            assert c2 == count and np.array_equal(i2, ref["index"][:m]), (name, m)
    assert seen["empty"] == 0 and seen["empty_v"] == 0
    if thin == 0:
        with np.errstate(invalid="ignore"):
            ok = ~np.isnan(R.wrapped(g["x"], inp.lx)) & ~np.isnan(g["v"]) & (g["v"] != np.inf)
        assert seen["everything"] == int(ok.sum()) < g["x"].size     # NaN is never selected, nor v = +inf: v < v_hi is strict
        assert 0 < seen["plain"] < seen["plain_to_lx"] and 0 < seen["straddling"]
        assert seen["plain"] + seen["straddling"] > 0


def test_host_select_leaves_what_lies_behind_the_count_alone(amd, crafted):
    inp, g = crafted
    sel = amd.engine.make_select((0.0, inp.lx), (V_LO, V_HI))
    L = amd._lib.load()
    ref = R.select(g, inp.lx, x_window=(0.0, inp.lx), v_window=(V_LO, V_HI))
    n = C.c_int64(-5)
    for m in (0, 1, ref["count"] - 1, ref["count"], ref["count"] + 1):
        index = np.full(m + 1, -77, dtype=np.int64)
        assert L.pic1dp_hip_host_select(C.byref(inp), C.byref(sel), g["x"].ctypes.data, g["v"].ctypes.data, g["x"].size, m, C.byref(n),
                                        index.ctypes.data) == 0
        k = min(m, ref["count"])
        assert n.value == ref["count"] and np.array_equal(index[:k], ref["index"][:k]) and np.all(index[k:] == -77), m


def test_host_select_argument_errors(amd, crafted):
    inp, g = crafted
    L = amd._lib.load()
    x, v, n = g["x"], g["v"], C.c_int64(-5)
    index = np.full(x.size, -77, dtype=np.int64)

    def call(sel, max_=4, inp_=inp, count=n, xp=x.ctypes.data, vp=v.ctypes.data):
        return L.pic1dp_hip_host_select(C.byref(inp_) if inp_ is not None else None, C.byref(sel) if sel is not None else None, xp, vp, x.size,
                                        max_, C.byref(count) if count is not None else None, index.ctypes.data)

    good = amd.engine.make_select()
    assert call(good) == 0 and n.value > 0
    n.value = -5
    index[:] = -77
    for field in ("x_lo", "x_hi", "v_lo", "v_hi"):
        bad = amd.engine.make_select()
        setattr(bad, field, math.nan)
        assert call(bad) == ERR_ARG
        assert "NaN" in L.pic1dp_hip_last_error().decode()
    assert call(good, max_=-1) == ERR_ARG and "negative" in L.pic1dp_hip_last_error().decode()
    assert call(None) == ERR_ARG and "null" in L.pic1dp_hip_last_error().decode()
    assert call(good, inp_=None) == ERR_ARG and call(good, count=None) == ERR_ARG
    assert call(good, xp=None) == ERR_ARG and call(good, vp=None) == ERR_ARG
    assert n.value == -5 and np.all(index == -77)            # nothing written


# ---------------------------------------------------------------------------
# the hash
# ---------------------------------------------------------------------------
def test_restated_mix64_is_splitmix64():
    known = (6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431, 16408922859458223821)
    got = R.hashes(5, key=1234567, origin=0)                 # splitmix64's outputs 0 ... 4 of state 1234567
    assert tuple(int(h) for h in got) == known
    assert tuple(R.mix64_int(1234567 + (c + 1) * 0x9E3779B97F4A7C15) for c in range(5)) == known
    assert int(R.hashes(1, key=2**64 - 1, origin=2**63)[0]) == R.mix64_int(2**64 - 1 + (2**63 + 1) * 0x9E3779B97F4A7C15)


def test_hash_thinning_equals_the_reference_and_keeps_a_sixteenth(amd):
    inp = amd.make_input(nparticle_max=16, nx=16)
    n, thin = 2**16, 2**60
    x = np.linspace(0.0, inp.lx, n, endpoint=False)
    v = np.zeros(n)
    sigma = math.sqrt(n * (1.0 / 16.0) * (15.0 / 16.0))
    for key in (0, 1, 12345):
        for origin in (0, 10**8):
            keep = R.mask(x, v, inp.lx, thin=thin, key=key, origin=origin)
            ref = np.nonzero(keep)[0]
            count, index = amd.host_select(inp, x, v, thin=thin, key=key, origin=origin)
            assert count == ref.size and np.array_equal(index, ref), (key, origin)
            dev = (ref.size - n / 16.0) / sigma
            print("hash thinning key %d origin %d: kept %d of %d (%.2f sigma)" % (key, origin, ref.size, n, dev))
            assert abs(dev) <= 4.0, (key, origin, ref.size)
    a = amd.host_select(inp, x, v, thin=thin, key=0)[1]
    b = amd.host_select(inp, x, v, thin=thin, key=1)[1]
    assert not np.array_equal(a, b)                          # the key names another sample


def test_every_sixteenth_marker_of_a_quiet_start_is_one_velocity_band(amd):
    """why thinning is a hash and not a stride: u_v of a quiet start is the bit reversal of g"""
    n = 2**14
    uv, _ = amd.load_uniforms(2, 0, n)
    stride = uv[np.arange(n) % 16 == 0]
    assert stride.size == n // 16 and np.all(stride < 1.0 / 16.0)
    kept = uv[R.hashes(n) < np.uint64(2**60)]
    occupied = np.unique(np.floor(kept * 16.0).astype(int))
    assert occupied.tolist() == list(range(16))
    print("stride 16: u_v in [%.4f, %.4f]; hashed sixteenth: %d markers over all 16 bands" % (stride.min(), stride.max(), kept.size))


def test_selection_in_two_halves_with_their_origins_is_the_whole(amd, crafted):
    inp, _ = crafted
    rng = np.random.default_rng(11)
    n = 5000
    x, v = rng.uniform(0.0, inp.lx, n), rng.normal(0.0, 2.0, n)
    kw = dict(x_window=(0.6 * inp.lx, 0.2 * inp.lx), v_window=(-1.0, 3.0), fraction=0.25, key=9)
    for g0 in (0, 777):
        whole = amd.host_select(inp, x, v, origin=g0, **kw)[1]
        lo = amd.host_select(inp, x[:n // 2], v[:n // 2], origin=g0, **kw)[1]
        hi = amd.host_select(inp, x[n // 2:], v[n // 2:], origin=g0 + n // 2, **kw)[1]
        assert 0 < lo.size and 0 < hi.size
        assert np.array_equal(np.concatenate([lo, hi + n // 2]), whole)
        assert np.array_equal(whole, np.nonzero(R.mask(x, v, inp.lx, kw["x_window"], kw["v_window"], R.thin_of(0.25), 9, g0))[0])
    assert not np.array_equal(amd.host_select(inp, x, v, origin=0, **kw)[1], amd.host_select(inp, x, v, origin=1, **kw)[1])


# ---------------------------------------------------------------------------
# the kernels' chunk plan
# ---------------------------------------------------------------------------
def test_chunk_plan_puts_every_marker_into_exactly_one_chunk(probe):
    cp = probe.host_select_plan(1, 256)["chunk_pairs"]
    assert cp >= 1024 and cp % 1024 == 0                     # whole trips of the largest workgroup, whole tiles' pairs
    cm = 2 * cp
    nt_edge = 288 * 1048576 // 16
    for num_cu in (8, 256):
        for np_ in (0, 1, 2, cm - 1, cm, cm + 1, 3 * cm + 1, nt_edge, nt_edge + 1, 10**8):
            s = probe.host_select_plan(np_, num_cu)
            print("select plan np %d, %d CUs: %s" % (np_, num_cu, s))
            assert s["chunk_pairs"] == cp and s["blocks"] >= 1 and s["threads"] % 64 == 0 and 64 <= s["threads"] <= 1024
            assert s["scan_threads"] % 64 == 0 and 64 <= s["scan_threads"] <= 1024
            assert s["nt"] == (16 * np_ > 288 * 1048576)
            npair, nchunk = np_ // 2, s["nchunk"]
            if np_ == 0:
                assert nchunk == 0
                continue
            assert nchunk == max(1, -(-npair // cp)) and s["blocks"] <= nchunk
            # chunk c: pairs [c cp, min((c + 1) cp, npair)); the odd last marker belongs to the last chunk
            first = np.arange(nchunk, dtype=np.int64) * cp
            last = np.minimum(first + cp, npair)
            assert first[0] == 0 and last[-1] == npair and np.array_equal(first[1:], last[:-1]) and np.all(last >= first)
            markers = 2 * (last - first)
            markers[-1] += np_ & 1
            assert int(markers.sum()) == np_ and (nchunk == 1 or np.all(markers[:-1] == cm))
            assert 0 < markers[-1] <= cm + 1
    assert not probe.host_select_plan(nt_edge, 256)["nt"] and probe.host_select_plan(nt_edge + 1, 256)["nt"]
    # a launch shape asked for by hand is taken literally; one the kernels cannot run is not
    s = probe.host_select_plan(10**8, 256, threads=64, blocks_per_cu=1)
    assert s["threads"] == 64 and s["blocks"] == 256
    s = probe.host_select_plan(10**8, 256, threads=1024, blocks_per_cu=4)
    assert s["threads"] == 1024 and s["blocks"] == 1024
    assert probe.host_select_plan(10**8, 256, threads=100)["threads"] == probe.host_select_plan(10**8, 256)["threads"]
    assert probe.host_select_plan(3 * cm + 1, 256, threads=256, blocks_per_cu=4)["blocks"] == 3


# ---------------------------------------------------------------------------
# the stand-alone program under the host sanitizers
# ---------------------------------------------------------------------------
def test_rule_under_the_host_sanitizers(tmp_path):
    """tests/select_check.cpp, a program of its own, built with AddressSanitizer and UndefinedBehaviorSanitizer (host code
    only; nothing of it touches a GPU): pic1dp_hip_host_select and pic1dp_hip_select_thin on the crafted markers"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pic1dp_amd_build", os.path.join(ROOT, "pic1dp_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    exe = str(tmp_path / "select_check")
    csrc = os.path.join(ROOT, "pic1dp_amd", "csrc")
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "select_check.cpp"), os.path.join(csrc, "select_host.cpp"),
                           "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failed"), r.stdout
