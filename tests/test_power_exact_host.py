"""The exact wave-particle power (include/pic1dp_hip.h pic1dp_hip_power_exact), the parts that need no GPU:
the quantum from the input and max |E|, the lengths and refusals, the conversion of limbs against Python integers, the pass
plan (through the probe library), the stand-alone checker under the host's sanitizers, and tests/power_exact.py's numpy
evaluation against its own plain-Python one."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import moments_exact as MX
import power_exact as PX
from conftest import ROOT

CAP = 150 * 1024                   # launch_policy.hpp kDiagLdsCap = 153 600
INF = math.inf


def tile(nx):
    return (8 * (nx + 1) + 15) // 16 * 16


# ---------------------------------------------------------------------------
# the quantum
# ---------------------------------------------------------------------------
def scale_cases():
    out = [0.0, 5e-324, 1e-300, 1.7976931348623157e308]
    for k in (-3, 0, 1, 10):
        p = 2.0 ** k
        out += [p, math.nextafter(p, INF), math.nextafter(p, -INF)]
    return out


@pytest.mark.parametrize("kw", [dict(), dict(v_max=8.000001), dict(v_max=0.5), dict(nparticle_max=10**7)])
def test_quantum_follows_the_rule(amd, kw):
    inp = amd.make_input(**dict(dict(nparticle_max=1000), **kw))
    kb, kvm = amd.charge_quantum(inp, 0) + 52, MX.ceil_log2(inp.v_max)
    want_kE = {0.0: 0, 5e-324: -1074, 1e-300: -996, 1.7976931348623157e308: 1024,
               0.125: -3, math.nextafter(0.125, INF): -2, math.nextafter(0.125, -INF): -3,
               1.0: 0, math.nextafter(1.0, INF): 1, math.nextafter(1.0, -INF): 0,
               2.0: 1, math.nextafter(2.0, INF): 2, math.nextafter(2.0, -INF): 1,
               1024.0: 10, math.nextafter(1024.0, INF): 11, math.nextafter(1024.0, -INF): 10}
    cases = scale_cases()
    assert sorted(cases) == sorted(want_kE)
    for m in cases:
        want = max(kb + kvm + want_kE[m] - 40, -1000)
        assert amd.power_quantum(inp, m) == want == PX.quantum(inp, m), m
    assert amd.power_quantum(inp, 1e-300) == -1000 and amd.power_quantum(inp, 5e-324) == -1000          # the clamp
    assert amd.power_quantum(inp, 0.0) == kb + kvm - 40 == amd.moments_quanta(inp, 0)[1]
    for bad in (math.nan, INF, -INF, -1.0):
        with pytest.raises(amd.Pic1dpError) as ei:
            amd.power_quantum(inp, bad)
        assert ei.value.code == 1 and "field not finite" in str(ei.value)
    with pytest.raises(amd.Pic1dpError) as ei:
        amd.power_quantum(inp, 1.0, ispecies=1)
    assert ei.value.code == 1
    L = amd._lib.load()
    assert L.pic1dp_hip_power_quantum(C.byref(inp), 0, 1.0, None) == 1 and L.pic1dp_hip_power_quantum(None, 0, 1.0, C.byref(C.c_int32())) == 1


# ---------------------------------------------------------------------------
# lengths and refusals
# ---------------------------------------------------------------------------
def test_limbs_len_and_refusals_by_name(amd):
    inp = amd.make_input(nparticle_max=10, nx_opd=64, nv_opd=64)
    assert [amd.power_limbs_len(inp, which) for which in (1, 2, 3)] == [2 * 4096 + 2, 2 * 4096 + 2, 2 * (2 * 4096 + 2)]
    small = amd.make_input(nparticle_max=10, nx_opd=1, nv_opd=2)
    assert [amd.power_limbs_len(small, which) for which in (1, 2, 3)] == [6, 6, 12]
    for which in (0, 4, -1):
        with pytest.raises(amd.Pic1dpError) as ei:
            amd.power_limbs_len(inp, which)
        assert ei.value.code == 1 and "which = %d" % which in str(ei.value)
    full = amd.make_input(nparticle_max=10, nx_opd=3, nv_opd=5, deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0])
    assert amd.power_limbs_len(full, 1) == 32
    for which in (2, 3):
        with pytest.raises(amd.Pic1dpError) as ei:
            amd.power_limbs_len(full, which)
        assert ei.value.code == 1 and "full-f" in str(ei.value) and "which = %d" % which in str(ei.value)
        with pytest.raises(amd.Pic1dpError) as ei:
            amd.power_convert(full, np.zeros(32 * (which - 1), dtype=np.int64), 0, which)
        assert ei.value.code == 1 and "full-f" in str(ei.value)
    for kw in (dict(nx_opd=0), dict(nv_opd=1)):
        bad = amd.make_input(nparticle_max=10)
        for k, val in kw.items():
            setattr(bad, k, val)
        with pytest.raises(amd.Pic1dpError) as ei:
            amd.power_limbs_len(bad, 1)
        assert ei.value.code == 1 and "nx_opd >= 1 and nv_opd >= 2" in str(ei.value)
    L = amd._lib.load()
    limbs, out = np.zeros(12, dtype=np.int64), np.zeros(10)
    assert L.pic1dp_hip_power_convert(C.byref(small), 3, 0, None, out.ctypes.data_as(C.c_void_p)) == 1 and b"null" in L.pic1dp_hip_last_error()
    assert L.pic1dp_hip_power_convert(C.byref(small), 3, 0, limbs.ctypes.data_as(C.c_void_p), None) == 1
    assert L.pic1dp_hip_power_convert(None, 3, 0, limbs.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 1
    assert L.pic1dp_hip_power_limbs_len(C.byref(small), 3, None) == 1 and L.pic1dp_hip_power_limbs_len(None, 3, C.byref(C.c_int64())) == 1
    assert L.pic1dp_hip_power_exact(None, 0, 1, None) == 1 and b"null context" in L.pic1dp_hip_last_error()
    assert L.pic1dp_hip_power_local_exact(None, 0, 1, None, None) == 1 and b"null context" in L.pic1dp_hip_last_error()
    with pytest.raises(ValueError):
        amd.power_convert(small, limbs[:6], 0, 3)


# ---------------------------------------------------------------------------
# the conversion
# ---------------------------------------------------------------------------
def split_unnormalised(total, rng, ranks):
    """(hi, lo) with hi 2^32 + lo == total: the element-wise sum of `ranks` normalised pairs"""
    parts = [int(rng.integers(-2**40, 2**40)) for _ in range(ranks - 1)]
    parts.append(total - sum(parts))
    his, los = zip(*(MX.limbs_of(t) for t in parts))
    return sum(his), sum(los)


@pytest.mark.parametrize("e", [0, -37, 11])
def test_convert_against_python_integers(amd, e):
    nxo, nvo = 4, 5
    nxv = nxo * nvo
    inp = amd.make_input(nparticle_max=1000, nx_opd=nxo, nv_opd=nvo)
    rng = np.random.default_rng(5)
    base = [0, 1, -1, 2**53 + 1, -(2**53 + 1), 2**53 + 3, -(2**53 + 3), 2**32, -(2**32), 2**32 - 1, -(2**32) + 1, 2**60, -(2**60),
            (2**44 - 1) * 2**19, 2**54 + 2, 2**54 + 6, -7, 2**53 - 1, 12345678901234567, -98765432109876543, 3 * 2**40]
    assert len(base) == nxv + 1
    assert float(2**53 + 1) == 2.0**53 and float(2**53 + 3) == 2.0**53 + 4                     # the ties go to even
    limbs = np.zeros((2, 2 * nxv + 2), dtype=np.int64)
    want = []
    for j in range(2):
        totals = [base[(b + 7 * j) % len(base)] for b in range(nxv)]
        rest = base[(nxv + 7 * j) % len(base)] * (-1 if j else 1)
        for b, t in enumerate(totals + [rest]):
            kind = (b + j) % 4
            if kind == 0:                                                  # normalised: negative hi where t < 0
                hi, lo = MX.limbs_of(t)
                assert 0 <= lo < 2**32 and (hi < 0) == (t < 0)
            elif kind == 1:                                                # as after summing two ranks
                hi, lo = split_unnormalised(t, rng, 2)
            elif kind == 2:                                                # ... eight ranks
                hi, lo = split_unnormalised(t, rng, 8)
            else:                                                          # lo beyond 2^32
                hi, lo = MX.limbs_of(t)
                hi, lo = hi - 5, lo + 5 * 2**32
            assert hi * 2**32 + lo == t
            if b < nxv:
                limbs[j, b], limbs[j, nxv + b] = hi, lo
            else:
                limbs[j, 2 * nxv], limbs[j, 2 * nxv + 1] = hi, lo
        assert PX.totals_of(limbs[j], nxv) == (totals, rest)
        want.append(PX.doubles_of(totals, rest, e, nxo, nvo))
    assert any(t < 0 for t in base)
    got = amd.power_convert(inp, limbs, e, 3)
    assert list(got) == ["total", "pertb"]
    for j, name in enumerate(got):
        assert got[name]["xv"].tobytes() == want[j]["xv"].tobytes() and got[name]["v"].tobytes() == want[j]["v"].tobytes()
        assert got[name]["rest"] == want[j]["rest"]
        assert got[name]["xv"].shape == (nvo, nxo) and got[name]["v"].shape == (nvo,)
    for which, name, j in ((1, "total", 0), (2, "pertb", 1)):
        one = amd.power_convert(inp, limbs[j:j + 1], e, which)
        assert list(one) == [name] and one[name]["xv"].tobytes() == want[j]["xv"].tobytes() and one[name]["rest"] == want[j]["rest"]
    z = amd.power_convert(inp, np.zeros((2, 2 * nxv + 2), dtype=np.int64), e, 3)
    assert not np.any(z["total"]["xv"]) and not np.any(z["pertb"]["v"]) and z["total"]["rest"] == 0.0


def test_v_profile_is_the_integer_row_sum(amd):
    """a plane where the sum of the converted bins differs from the converted sum: three bins of 2^53 + 1 quanta convert to
    2^53 each, their integer sum 3 2^53 + 3 converts to 3 2^53 + 4"""
    nxo, nvo = 3, 2
    inp = amd.make_input(nparticle_max=1000, nx_opd=nxo, nv_opd=nvo)
    totals = [2**53 + 1] * 3 + [2**53 + 1, -(2**53 + 3), 5]
    limbs = PX.pack(totals, 0)[None, :]
    for e in (0, -20):
        got = amd.power_convert(inp, limbs, e, 1)["total"]
        q = math.ldexp(1.0, e)
        assert got["xv"][0].tolist() == [2.0**53 * q] * 3
        assert got["v"][0] == (3 * 2.0**53 + 4) * q != float(np.sum(got["xv"][0]))
        assert got["v"][1] == float(2**53 + 1 - (2**53 + 3) + 5) * q == 3.0 * q
        assert got["v"].tobytes() == PX.doubles_of(totals, 0, e, nxo, nvo)["v"].tobytes()


# ---------------------------------------------------------------------------
# the pass plan
# ---------------------------------------------------------------------------
def exact_blocks(np_, cu):
    return max(1, min(cu, -(-np_ // 2**17)))


def test_plan_is_the_power_plan_with_the_exact_grid(probe):
    # power_plan's three branches at the issue's grids ...
    n = 200_000
    for (nx, nxo, nvo), want in (((1024, 64, 64), [(8208 + 65536, 3, 1, 0, 2)]),
                                 ((8192, 96, 96), [(139280, 1, 1, 0, 1), (139280, 2, 1, 1, 1)]),
                                 ((64, 160, 160), [(528, 3, 0, 0, 2)])):
        pl = probe.host_power_plan_exact(nx, nxo, nvo, 3, 1, n, 256)
        assert [(ps["bytes"], ps["sets"], ps["lds"], ps["first_set"], ps["nsets"]) for ps in pl["passes"]] == want
        assert all(ps["blocks"] == 2 and ps["threads"] == 1024 and ps["nt"] == 0 for ps in pl["passes"])
    # ... and at the exact byte of every flip (nx 1023: the tile is 8192 B; nv_opd 2: a plane is 16 nx_opd B)
    nx, room = 1023, CAP - 8192
    assert tile(nx) == 8192 and 2 * 16 * 4544 == room and 16 * 9088 == room
    pl = probe.host_power_plan_exact(nx, 4544, 2, 3, 1, n, 256)
    assert [(ps["bytes"], ps["lds"], ps["sets"]) for ps in pl["passes"]] == [(CAP, 1, 3)]
    pl = probe.host_power_plan_exact(nx, 4545, 2, 3, 1, n, 256)
    assert [(ps["bytes"], ps["sets"], ps["lds"], ps["first_set"]) for ps in pl["passes"]] == [(8192 + 72720, 1, 1, 0), (8192 + 72720, 2, 1, 1)]
    for which, npass in ((3, 2), (2, 1), (1, 1)):
        pl = probe.host_power_plan_exact(nx, 9088, 2, which, 1, n, 256)
        assert [(ps["bytes"], ps["lds"]) for ps in pl["passes"]] == [(CAP, 1)] * npass
        pl = probe.host_power_plan_exact(nx, 9089, 2, which, 1, n, 256)
        assert [(ps["bytes"], ps["lds"], ps["nsets"]) for ps in pl["passes"]] == [(8192, 0, npass)]
    assert len(probe.host_power_plan_exact(1024, 4544, 2, 3, 1, n, 256)["passes"]) == 2       # the tile's own 16 bytes
    # everything but the grid is power_plan's
    for nx_ in (1, 2, 64, 1023, 1024, 8192):
        for nxo, nvo in ((1, 2), (3, 5), (64, 64), (96, 96), (160, 160), (4545, 2), (9089, 2)):
            for which in (1, 2, 3):
                for deltaf in (0, 1):
                    for np_ in (0, 1, 2**17, 2**17 + 1, 10**8):
                        for cu in (8, 256):
                            base = probe.host_power_plan(nx_, nxo, nvo, which, deltaf, np_, cu)
                            got = probe.host_power_plan_exact(nx_, nxo, nvo, which, deltaf, np_, cu)
                            assert {k: got[k] for k in ("selected", "tile", "plane")} == {k: base[k] for k in ("selected", "tile", "plane")}
                            assert len(got["passes"]) == len(base["passes"])
                            for a, b in zip(got["passes"], base["passes"]):
                                assert {k: a[k] for k in a if k != "blocks"} == {k: b[k] for k in b if k != "blocks"}
                                assert a["blocks"] == exact_blocks(np_, cu)
                                assert a["bytes"] == got["tile"] + (a["nsets"] * got["plane"] if a["lds"] else 0) <= CAP
    # the grid
    blocks = lambda np_, cu=256: [ps["blocks"] for ps in probe.host_power_plan_exact(64, 64, 64, 3, 1, np_, cu)["passes"]]   # noqa: E731
    assert [blocks(np_) for np_ in (1, 2**17, 2**17 + 1, 256 * 2**17 + 1)] == [[1], [1], [2], [256]]
    assert blocks(255 * 2**17 + 1) == [256] and blocks(255 * 2**17) == [255] and blocks(0) == [1] and blocks(10**8, 8) == [8]
    assert probe.host_power_plan_exact(64, 64, 64, 2, 0, 1000, 256)["passes"] == [] and probe.host_power_plan_exact(64, 64, 64, 0, 1, 1000, 256)["passes"] == []


# ---------------------------------------------------------------------------
# the stand-alone checker
# ---------------------------------------------------------------------------
def test_host_arithmetic_under_the_host_sanitizers(tmp_path):
    """tests/power_fx_check.cpp, a program of its own, built with AddressSanitizer and UndefinedBehaviorSanitizer (host code
    only; nothing of it touches a GPU): csrc/power_fx.cpp against __int128 arithmetic, and the device's ceil(log2) from the
    bits against the host's at powers of two, their neighbours and 2 10^5 random doubles"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pic1dp_amd_build", os.path.join(ROOT, "pic1dp_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    exe = str(tmp_path / "power_fx_check")
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "power_fx_check.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failed"), r.stdout


# ---------------------------------------------------------------------------
# declared, bound, documented
# ---------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_documented(amd, probe):
    lib = C.CDLL(amd._lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pic1dp_hip.h")).read()
    mod = open(os.path.join(ROOT, "pic1dp_amd", "fortran", "pic1dp_hip_mod.F90")).read()
    for name in ("power_quantum", "power_limbs_len", "power_local_exact", "power_convert", "power_exact", "power_exact_stats"):
        assert hasattr(lib, "pic1dp_hip_" + name), name
        assert "pic1dp_hip_" + name in amd._lib.SIGNATURES, name
        assert re.search(r"\bint pic1dp_hip_%s\(" % name, header), name
        assert 'bind(C, name="pic1dp_hip_%s")' % name in mod, name
    assert callable(amd.Pic1dp.power_exact) and callable(amd.Pic1dp.power_local_exact) and callable(amd.Pic1dp.power_exact_stats)
    for name in ("power_quantum", "power_limbs_len", "power_convert"):
        assert callable(getattr(amd, name)) and name in amd.__all__
    assert callable(probe.host_power_plan_exact)
    assert "pic1dp_probe_host_power_plan_exact" in open(os.path.join(ROOT, "include", "pic1dp_probe.h")).read()
    for line in ("e = max(kb + kvm + kE - 40, -1000)", "n = rint(t 2^-e)", "[hi plane: nv_opd * nx_opd | lo plane: nv_opd * nx_opd | rest hi | rest lo]",
                 "int pic1dp_hip_power_exact_stats(pic1dp_ctx *ctx, double *ms, int64_t *passes, int64_t *rejected);", "field not finite"):
        assert line in header, line
    assert "There is no exact" not in header


# ---------------------------------------------------------------------------
# the reference module against itself
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nxo,nvo", [(2, 1, 2), (3, 3, 5), (8, 6, 4)])
def test_reference_equals_a_marker_by_marker_evaluation(amd, nx, nxo, nvo):
    inp = amd.make_input(nparticle_max=1000, nx=nx, nx_opd=nxo, nv_opd=nvo)
    rng = np.random.default_rng(nx + nxo)
    n = 300
    x = rng.uniform(-1.0, 2.0, n) * inp.lx
    v = rng.normal(0.0, 0.6 * inp.v_max, n)
    x[:3], v[:3] = [0.0, inp.lx, -0.0], [0.0, math.nextafter(inp.v_max, 0.0), -inp.v_max]
    assert np.count_nonzero(np.abs(v) >= inp.v_max) > 5
    p, w = rng.uniform(0.5, 1.5, n), rng.normal(0.0, 0.1, n)
    x[5], v[5], w[5], v[6] = 0.3 * inp.lx, 0.3 * inp.v_max, 1e200, 1e200     # four binned terms of w and a rest term of each set: not summed, counted
    E = rng.normal(0.0, 1.0, nx) + 0.25
    ref = PX.reference(x, v, p, w, E, inp, which=3)
    assert ref["e"] == PX.quantum(inp, float(np.abs(E).max())) == amd.power_quantum(inp, float(np.abs(E).max()))
    assert ref["rejected"].tolist() == [[0, 1], [4, 1]]
    nxv = nxo * nvo
    for j, q in enumerate((p, w)):
        totals, rest, rejected = PX.python_limbs(x, v, q, E, inp, ref["e"])
        assert ref["rejected"][j].tolist() == rejected
        assert ref["totals"][j] == totals and ref["rest"][j] == rest
        assert PX.totals_of(ref["limbs"][j], nxv) == (totals, rest)
        assert np.all((ref["limbs"][j, nxv:2 * nxv] >= 0) & (ref["limbs"][j, nxv:2 * nxv] < 2**32)) and 0 <= ref["limbs"][j, -1] < 2**32
    ok = np.ones(n, dtype=bool)
    ok[5:7] = False
    r2 = PX.reference(x[ok], v[ok], p[ok], w[ok], E, inp, which=3)
    assert PX.in_range(r2) and not PX.in_range(ref)
    for which, j in ((1, 0), (2, 1)):
        r1 = PX.reference(x[ok], v[ok], p[ok], w[ok], E, inp, which=which)
        assert list(r1["doubles"]) == [PX.SETS[j]] and r1["limbs"].tobytes() == r2["limbs"][j:j + 1].tobytes()
    # the converted doubles are the library's conversion of the limbs
    got = amd.power_convert(inp, r2["limbs"], r2["e"], 3)
    for name in PX.SETS:
        for key in ("xv", "v"):
            assert got[name][key].tobytes() == r2["doubles"][name][key].tobytes(), (name, key)
        assert got[name]["rest"] == r2["doubles"][name]["rest"]
