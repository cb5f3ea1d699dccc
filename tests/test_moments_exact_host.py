"""The exact velocity moments (include/pic1dp_hip.h pic1dp_hip_moments_exact), the parts that need no GPU: the
quanta, the conversion of limbs, the lengths and refusals, the pass plan (through the probe library) and
tests/moments_exact.py's numpy evaluation against its own plain-Python one."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import moments_exact as MX
from conftest import ROOT
from test_moments_host import crafted

TWO = dict(nspecies=2, species_charge=[-1.0, 1.0], species_mass=[1.0, 4.0], species_temperature=[1.0, 1.0],
           species_temperature2=[1.0, 1.0], species_density=[0.9, 0.9], species_v0=[5.0, 5.0])


# ---------------------------------------------------------------------------
# the quanta
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw,kvm", [(dict(), None), (dict(v_max=0.3), -1), (dict(v_max=0.5), -1), (dict(v_max=0.51), 0),
                                    (dict(v_max=1.0), 0), (dict(v_max=8.0), 3), (dict(v_max=8.000001), 4), (dict(v_max=6.0), 3),
                                    (dict(v_max=2.0 ** -7), -7), (dict(nparticle_max=10**7), None)])
def test_quanta_follow_the_formula(amd, kw, kvm):
    inp = amd.make_input(**dict(dict(nparticle_max=1000), **kw))
    if kvm is None:
        kvm = math.ceil(math.log2(inp.v_max))
    assert MX.ceil_log2(inp.v_max) == kvm
    e = amd.moments_quanta(inp, 0)
    assert e == [amd.charge_quantum(inp, 0) + 52 + k * kvm - 40 for k in range(4)]
    assert e == MX.quanta(inp, 0)


def test_quanta_of_two_species_with_unequal_bounds(amd):
    inp = amd.make_input(nparticle_max=1000, species_nparticle_init=[1000, 37], **TWO)
    q = [amd.charge_quantum(inp, s) for s in range(2)]
    assert q[0] != q[1]
    kvm = MX.ceil_log2(inp.v_max)
    for s in range(2):
        assert amd.moments_quanta(inp, s) == [q[s] + 12 + k * kvm for k in range(4)]
    with pytest.raises(amd.Pic1dpError) as ei:
        amd.moments_quanta(inp, 2)
    assert ei.value.code == 1
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(amd.Pic1dpError) as ei:
            amd.moments_quanta(amd.make_input(nparticle_max=1000, v_max=bad), 0)
        assert ei.value.code == 1          # (v_max by name, unless the bound on the weights is refused first)


# ---------------------------------------------------------------------------
# the conversion
# ---------------------------------------------------------------------------
def split_unnormalised(total, rng, ranks):
    """(hi, lo) int64 with hi 2^32 + lo == total: the element-wise sum of `ranks` normalised pairs"""
    parts = [int(rng.integers(-2**40, 2**40)) for _ in range(ranks - 1)]
    parts.append(total - sum(parts))
    his, los = zip(*(MX.limbs_of(t) for t in parts))
    return sum(his), sum(los)


def test_convert_against_python_integers(amd):
    nx = 16
    inp = amd.make_input(nparticle_max=1000, nx=nx)
    e = amd.moments_quanta(inp, 0)
    rng = np.random.default_rng(5)
    totals = [0, 1, -1, 2**53 + 1, -(2**53 + 1), 2**53 + 3, -(2**53 + 3), 2**32, -(2**32), 2**32 - 1, -(2**32) + 1, 2**60, -(2**60),
              (2**44 - 1) * 2**18, 2**54 + 2, 2**54 + 6]
    assert len(totals) == nx
    assert float(2**53 + 1) == 2.0**53 and float(2**53 + 3) == 2.0**53 + 4         # the ties go to even
    limbs = np.zeros((2, 4, 2, nx), dtype=np.int64)
    want = np.zeros((2, 4, nx))
    for j in range(2):
        for k in range(4):
            for b in range(nx):
                t = totals[(b + k + 4 * j) % nx]
                kind = (b + j) % 4
                if kind == 0:                                                  # normalised: negative hi where t < 0
                    hi, lo = MX.limbs_of(t)
                    assert 0 <= lo < 2**32 and (hi < 0) == (t < 0)
                elif kind == 1:                                                # as after summing 3 ranks
                    hi, lo = split_unnormalised(t, rng, 3)
                elif kind == 2:                                                # lo >= 2^32
                    hi, lo = MX.limbs_of(t)
                    hi, lo = hi - 5, lo + 5 * 2**32
                    assert lo >= 2**32
                else:                                                          # many ranks: lo far beyond 2^32
                    hi, lo = split_unnormalised(t, rng, 1000)
                assert hi * 2**32 + lo == t
                limbs[j, k, 0, b], limbs[j, k, 1, b] = hi, lo
                want[j, k, b] = MX.to_double(t, e[k])
    got = amd.moments_convert(inp, limbs, 3)
    assert list(got) == ["total", "pertb"]
    assert got["total"].tobytes() == want[0].tobytes() and got["pertb"].tobytes() == want[1].tobytes()
    for which, name, j in ((1, "total", 0), (2, "pertb", 1)):
        one = amd.moments_convert(inp, limbs[j:j + 1], which)
        assert list(one) == [name] and one[name].tobytes() == want[j].tobytes()
    assert not np.any(amd.moments_convert(inp, np.zeros((2, 4, 2, nx), dtype=np.int64), 3)["total"])


def test_limb_arithmetic_under_the_host_sanitizers(tmp_path):
    """tests/fx_limbs_check.cpp, a program of its own, built with AddressSanitizer and UndefinedBehaviorSanitizer (host code
    only; nothing of it touches a GPU): csrc/fx_limbs.hpp against __int128 arithmetic"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pic1dp_amd_build", os.path.join(ROOT, "pic1dp_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    exe = str(tmp_path / "fx_limbs_check")
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "fx_limbs_check.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failed"), r.stdout


# ---------------------------------------------------------------------------
# lengths and refusals
# ---------------------------------------------------------------------------
def test_limbs_len_and_refusals_by_name(amd):
    assert [amd.moments_limbs_len(which, 192) for which in (1, 2, 3)] == [8 * 192, 8 * 192, 16 * 192]
    assert amd.moments_limbs_len(3, 1) == 16
    for which, nx in ((0, 192), (4, 192), (-1, 192), (1, 0)):
        with pytest.raises(amd.Pic1dpError) as ei:
            amd.moments_limbs_len(which, nx)
        assert ei.value.code == 1 and "moments_limbs_len" in str(ei.value)
    inp = amd.make_input(nparticle_max=1000, nx=8)
    limbs = np.zeros((2, 4, 2, 8), dtype=np.int64)
    for which in (0, 4):
        with pytest.raises(amd.Pic1dpError) as ei:
            amd._lib.check(amd._lib.load().pic1dp_hip_moments_convert(C.byref(inp), 0, which, limbs.ctypes.data_as(C.c_void_p),
                                                                      np.zeros((2, 4, 8)).ctypes.data_as(C.c_void_p)))
        assert ei.value.code == 1 and "which = %d" % which in str(ei.value)
    with pytest.raises(amd.Pic1dpError) as ei:
        amd.moments_convert(inp, limbs, 3, ispecies=1)
    assert ei.value.code == 1
    full_f = amd.make_input(nparticle_max=1000, nx=8, deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0])
    for which in (2, 3):
        with pytest.raises(amd.Pic1dpError) as ei:
            amd.moments_convert(full_f, limbs[:1 if which == 2 else 2], which)
        assert ei.value.code == 1 and "full-f" in str(ei.value) and "which = %d" % which in str(ei.value)
    assert list(amd.moments_convert(full_f, limbs[:1], 1)) == ["total"]
    out = np.zeros((2, 4, 8))
    L = amd._lib.load()
    assert L.pic1dp_hip_moments_convert(C.byref(inp), 0, 3, None, out.ctypes.data_as(C.c_void_p)) == 1
    assert L.pic1dp_hip_moments_convert(C.byref(inp), 0, 3, limbs.ctypes.data_as(C.c_void_p), None) == 1
    assert L.pic1dp_hip_moments_convert(None, 0, 3, limbs.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 1
    assert L.pic1dp_hip_moments_limbs_len(3, 8, None) == 1 and L.pic1dp_hip_moments_quanta(C.byref(inp), 0, None) == 1
    with pytest.raises(ValueError):
        amd.moments_convert(inp, limbs[:1], 3)


# ---------------------------------------------------------------------------
# the pass plan
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [2, 3, 77, 192, 1024, 2048, 2049, 4096, 4800, 4801, 8192])
def test_plan_is_the_moments_plan_with_the_exact_grid(probe, nx):
    for which in (1, 2, 3):
        for deltaf in (0, 1):
            for np_ in (0, 1, 2**17, 2**17 + 1, 10**8):
                for cu in (8, 256):
                    base = probe.host_moments_plan(nx, which, deltaf, np_, cu)
                    got = probe.host_moments_plan_exact(nx, which, deltaf, np_, cu)
                    assert got["selected"] == base["selected"] and got["group"] == base["group"]
                    assert len(got["passes"]) == len(base["passes"])
                    blocks = max(1, min(cu, -(-np_ // 2**17)))
                    for a, b in zip(got["passes"], base["passes"]):
                        assert {k: a[k] for k in a if k != "blocks"} == {k: b[k] for k in b if k != "blocks"}
                        assert a["blocks"] == blocks, (nx, which, np_, cu)
    assert [probe.host_moments_plan_exact(nx, 1, 1, n, 256)["passes"][0]["blocks"] for n in (0, 1, 2**17, 2**17 + 1, 10**8)] == [1, 1, 1, 2, 256]
    assert [probe.host_moments_plan_exact(nx, 1, 1, n, 8)["passes"][0]["blocks"] for n in (0, 1, 2**17, 2**17 + 1, 10**8)] == [1, 1, 1, 2, 8]
    assert probe.host_moments_plan_exact(nx, 2, 0, 1000, 256)["passes"] == [] and probe.host_moments_plan_exact(nx, 0, 1, 1000, 256)["passes"] == []


# ---------------------------------------------------------------------------
# declared, bound, documented
# ---------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_documented(amd, probe):
    lib = C.CDLL(amd._lib.LIB_PATH)
    for name in ("moments_quanta", "moments_limbs_len", "moments_local_exact", "moments_convert", "moments_exact"):
        assert hasattr(lib, "pic1dp_hip_" + name), name
        assert "pic1dp_hip_" + name in amd._lib.SIGNATURES, name
    assert callable(amd.Pic1dp.moments_exact) and callable(amd.Pic1dp.moments_local_exact)
    for name in ("moments_quanta", "moments_convert", "moments_limbs_len"):
        assert callable(getattr(amd, name)) and name in amd.__all__
    assert callable(probe.host_moments_plan_exact)
    header = open(os.path.join(ROOT, "include", "pic1dp_hip.h")).read()
    for line in ("e[k] = kb + k * kvm - 40", "n = rint(t 2^-e[k])", "limbs[((j * 4 + k) * 2 + h) * nx + ix]", "which = 17", "which = 18",
                 "kvm = ceil(log2 v_max)"):
        assert line in header, line
    assert "There is no exact (fixed-quanta) kind" not in header
    mod = open(os.path.join(ROOT, "pic1dp_amd", "fortran", "pic1dp_hip_mod.F90")).read()
    for name in ("moments_quanta", "moments_limbs_len", "moments_local_exact", "moments_convert", "moments_exact"):
        assert 'bind(C, name="pic1dp_hip_%s")' % name in mod, name


# ---------------------------------------------------------------------------
# the reference module against itself
# ---------------------------------------------------------------------------
def test_quantise_py_rounds_to_even_and_rejects_at_the_limit():
    q = MX.quantise_py
    assert [q(t, 0) for t in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, 0.0, -0.0)] == [0, 2, 2, 0, -2, -2, 0, 0, 0]
    assert q(3.0, 1) == 2 and q(5.0, 1) == 2 and q(7.0, 1) == 4 and q(0.375, -2) == 2 and q(0.625, -2) == 2
    assert q(float(2**44 - 1), 0) == 2**44 - 1 and q(-float(2**44 - 1), 0) == -(2**44 - 1)
    assert q(float(2**44), 0) is None and q(-float(2**44), 0) is None
    below = math.nextafter(2.0**44 - 0.5, 0.0)
    assert q(below, 0) == 2**44 - 1 and q(2.0**44 - 0.5, 0) is None               # the tie goes to the even 2^44: not summed
    assert q(math.nan, 0) is None and q(math.inf, 0) is None and q(1e100, 0) is None and q(1e-320, -10) == 0
    assert q(math.ldexp(2**44 - 1, -300), -300) == 2**44 - 1 and q(math.ldexp(1.0, 300), 300 - 44) is None
    for t, e in ((1.1, -30), (-2.7e5, -3), (3.3e-7, -60), (2.5, 0), (-3.5, 0)):
        r, ok = MX.quantise(np.array([t]), e)
        assert ok[0] and int(r[0]) == q(t, e)
    r, ok = MX.quantise(np.array([math.nan, 1e100, 2.0**44, -2.0**44, 2.0**44 - 0.5, below]), 0)
    assert ok.tolist() == [False, False, False, False, False, True]
    assert MX.limbs_of(-1) == (-1, 2**32 - 1) and MX.limbs_of(2**32) == (1, 0) and MX.limbs_of(0) == (0, 0)
    assert MX.to_double(2**53 + 1, -3) == 2.0**50 and MX.to_double(-(2**53 + 3), 0) == -(2.0**53 + 4)


@pytest.mark.parametrize("nx", [2, 3, 8])
def test_reference_equals_a_marker_by_marker_evaluation(amd, nx):
    inp = amd.make_input(nparticle_max=1000, nx=nx)
    x, v, p, w = crafted(inp)            # (1e100 among the velocities: terms that are not summed, and counted)
    e = MX.quanta(inp, 0)
    scale = 2.0 ** (e[0] + 40 - 3)       # the crafted weights reach 4.2: within the input's bound 2^kb (exact scaling)
    p, w = p * scale, w * scale
    ref = MX.reference(x, v, p, w, inp, which=3)
    assert ref["e"] == e and ref["limbs"].shape == (2, 4, 2, nx) and int(ref["count"].sum()) == 2 * x.size
    assert np.any(ref["rejected"]) and not np.any(ref["rejected"][:, 0])
    for j, q in enumerate((p, w)):
        totals, rejected = MX.python_limbs(x, v, q, inp, e)
        assert ref["rejected"][j].tolist() == rejected
        for k in range(4):
            assert ref["totals"][j][k] == totals[k], (j, k)
            for b in range(nx):
                hi, lo = int(ref["limbs"][j, k, 0, b]), int(ref["limbs"][j, k, 1, b])
                assert 0 <= lo < 2**32 and hi * 2**32 + lo == totals[k][b]
                assert ref["doubles"][SETNAME[j]][k, b] == float(totals[k][b]) * 2.0 ** e[k]
    # in range: the velocities within 2 v_max
    ok = np.abs(v) <= 2.0 * inp.v_max
    r2 = MX.reference(x[ok], v[ok], p[ok], w[ok], inp, which=3)
    assert MX.in_range(r2)
    for which, j in ((1, 0), (2, 1)):
        r1 = MX.reference(x[ok], v[ok], p[ok], w[ok], inp, which=which)
        assert list(r1["doubles"]) == [SETNAME[j]] and r1["limbs"].tobytes() == r2["limbs"][j:j + 1].tobytes()
    # the converted doubles are the library's conversion of the limbs
    got = amd.moments_convert(inp, r2["limbs"], 3)
    for name in SETNAME:
        assert got[name].tobytes() == r2["doubles"][name].tobytes()


SETNAME = ("total", "pertb")
