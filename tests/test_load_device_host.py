"""The on-device particle load on the host: no GPU.  tests/load_reference.py restates the definition in
numpy and Python integers; the library's host_load_uniforms and load_origin are held against it, the launch shape of the
kernel's pass is pinned through the probe library, and tests/load_seq_check.cpp runs the definition's host unit under the
host sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import load_reference as R
from conftest import ROOT

ERR_ARG = 1


def test_restatement_reproduces_the_published_splitmix64_outputs():
    got = R.draws(R.KNOWN_KEY, np.arange(5, dtype=np.uint64))
    assert tuple(int(v) for v in got) == R.KNOWN_DRAWS
    z = R.KNOWN_KEY
    for c in range(5):
        assert R.mix64_int(z + (c + 1) * R.GOLD) == R.KNOWN_DRAWS[c]


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("g0", [0, 2**32 - 3, 2**33 + 1, 3**21 - 8])
def test_host_uniforms_equal_the_restatement_bit_for_bit(amd, kind, g0):
    n = 16 if kind == 1 or g0 + 16 <= 3**21 else 8
    for s in (0, 1):
        uv, ux = amd.load_uniforms(kind, g0, n, ispecies=s)
        ruv, rux = R.uniforms(kind, range(g0, g0 + n), 0, s)
        assert uv.tobytes() == ruv.tobytes() and ux.tobytes() == rux.tobytes()
        assert (uv >= 0).all() and (uv < 1).all() and (ux >= 0).all() and (ux < 1).all()
    if kind == 1:   # an ensemble member and a species are other streams
        a, b, c = (amd.load_uniforms(1, g0, n, seed_offset=o, ispecies=s)[0] for o, s in ((0, 0), (1, 0), (0, 1)))
        assert not (a == b).any() and not (a == c).any()
        uv, ux = amd.load_uniforms(1, g0, n, seed_offset=5, ispecies=1)
        ruv, rux = R.uniforms(1, range(g0, g0 + n), 5, 1)
        assert uv.tobytes() == ruv.tobytes() and ux.tobytes() == rux.tobytes()
    else:           # the same sequence for every species
        assert amd.load_uniforms(2, g0, n, ispecies=0)[1].tobytes() == amd.load_uniforms(2, g0, n, ispecies=1)[1].tobytes()


def test_known_quiet_start_values(amd):
    assert R.r3_int(1) == 3**20 and R.r3_int(3**21 - 1) == 3**21 - 1
    uv, ux = amd.load_uniforms(2, 0, 4)
    assert uv.tolist() == [0.0, 0.5, 0.25, 0.75]
    assert ux.tolist() == [0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0 / 9.0]
    uv, ux = amd.load_uniforms(2, 3**21 - 1, 1)
    assert ux[0] == np.float64(3**21 - 1) / np.float64(3**21)
    assert uv[0] == float(R.bitrev64_int(3**21 - 1) >> 11) * 2.0**-53


@pytest.mark.parametrize("npe", [1, 3, 4])
def test_load_origin_is_the_running_sum_of_the_blocks_valid_markers(amd, npe):
    inp = amd.make_input(nparticle_max=10_007, nspecies=2, species_nparticle_init=[10_001, 9_998], species_charge=[-1.0, 1.0],
                         species_mass=[1.0, 4.0], species_temperature=[1.0, 1.0], species_temperature2=[1.0, 1.0],
                         species_density=[0.9, 0.9], species_v0=[5.0, 5.0])
    assert 10_007 % npe or npe == 1
    import ctypes as C
    for s in (0, 1):
        total = 0
        for b in range(npe):
            assert amd.load_origin(inp, s, rank=b, nranks=npe) == total == R.origin(inp, s, b, npe, npe)
            na, npv = C.c_int64(), C.c_int64()
            assert amd._lib.load().pic1dp_hip_block_sizes(C.byref(inp), s, b, npe, C.byref(na), C.byref(npv)) == 0
            assert npv.value == R.block_np(inp, s, b, npe)
            total += npv.value
        assert total == inp.species_nparticle_init[s]
    if npe == 4:    # one process that owns two of the four blocks starts where its first block does
        assert amd.load_origin(inp, 0, rank=1, nranks=2, npe=4) == R.origin(inp, 0, 1, 2, 4) == amd.load_origin(inp, 0, rank=2, nranks=4)


def test_argument_errors(amd):
    for kind in (0, 3):
        with pytest.raises(amd.Pic1dpError) as ei:
            amd.load_uniforms(kind, 0, 4)
        assert ei.value.code == ERR_ARG and "kind" in str(ei.value)
    with pytest.raises(amd.Pic1dpError) as ei:
        amd.load_uniforms(2, 0, 4, seed_offset=1)
    assert ei.value.code == ERR_ARG and "seed offset" in str(ei.value)
    with pytest.raises(amd.Pic1dpError) as ei:
        amd.load_uniforms(2, 3**21 - 8, 9)          # the last one would be marker 3^21
    assert ei.value.code == ERR_ARG and "3^21" in str(ei.value)
    amd.load_uniforms(2, 3**21 - 8, 8)
    amd.load_uniforms(1, 3**21 - 8, 9)              # kind 1 has no such limit
    with pytest.raises(amd.Pic1dpError):
        amd.load_uniforms(1, -1, 4)
    for isp in (-1, 8):
        with pytest.raises(amd.Pic1dpError) as ei:
            amd.load_uniforms(1, 0, 4, ispecies=isp)
        assert ei.value.code == ERR_ARG and "species" in str(ei.value)
    amd.load_uniforms(1, 0, 4, ispecies=7)
    with pytest.raises(amd.Pic1dpError):
        amd.load_uniforms(1, 0, 4, seed_offset=-1)
    # more than 3^21 markers of a species: the origin is still defined (no allocation anywhere), the sequence ends
    big = amd.make_input(nparticle_max=3**21 + 5, species_nparticle_init=[3**21 + 1])
    g0 = amd.load_origin(big, 0, rank=1, nranks=2)
    assert g0 == R.origin(big, 0, 1, 2, 2) > 2**32
    with pytest.raises(amd.Pic1dpError):
        amd.load_uniforms(2, g0, 3**21 + 1 - g0)
    with pytest.raises(amd.Pic1dpError):
        amd.load_origin(big, 1)                     # bad species index


def test_load_launch_covers_every_slot_once_and_starts_no_empty_workgroup(probe):
    nt_edge = 288 * 1048576 // 32                   # 32 B written per slot against diag_launch's threshold
    for num_cu in (8, 256):
        for nalloc in (1, 2, 4095, 4096, 4097, 2 * 4096 + 1, 100_001, 8 * 256 * 4096, 8 * 256 * 4096 + 1, nt_edge, nt_edge + 1, 10**8):
            l = probe.host_load_launch(nalloc, num_cu)
            assert l["threads"] == 256 and l["chunk"] == 4096
            nchunk = -(-nalloc // l["chunk"])
            assert 1 <= l["blocks"] <= nchunk                      # every workgroup has a first chunk
            assert l["blocks"] == min(nchunk, 8 * num_cu)
            # chunks b, b + blocks, ...: each chunk is taken by exactly one workgroup, and the chunks tile [0, nalloc)
            owner = np.arange(nchunk) % l["blocks"]
            assert np.bincount(owner, minlength=l["blocks"]).min() >= 1
            assert (nchunk - 1) * l["chunk"] < nalloc <= nchunk * l["chunk"]
            assert l["nt"] == (32 * nalloc > 288 * 1048576)
    assert not probe.host_load_launch(nt_edge, 256)["nt"] and probe.host_load_launch(nt_edge + 1, 256)["nt"]


def test_definition_under_the_host_sanitizers(tmp_path):
    """tests/load_seq_check.cpp, a program of its own, built with AddressSanitizer and UndefinedBehaviorSanitizer (host
    code only; nothing of it touches a GPU)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pic1dp_amd_build", os.path.join(ROOT, "pic1dp_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    exe = str(tmp_path / "load_seq_check")
    csrc = os.path.join(ROOT, "pic1dp_amd", "csrc")
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "load_seq_check.cpp"), os.path.join(csrc, "load_seq.cpp"),
                           os.path.join(csrc, "loader.cpp"), os.path.join(csrc, "multirand.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failed"), r.stdout


def test_fortran_host_refuses_a_word_that_is_no_load(tmp_path):
    """PIC1DP_LOAD is read before the context is created, so the refusal needs no device: words that only begin like one of
    host, random, quiet, another letter case, the empty word and one longer than the host's buffer all stop the run"""
    import shutil
    exe = os.path.join(ROOT, "pic1dp_amd", "fortran", "pic1dp_host")
    if not os.path.exists(exe):
        r = subprocess.run(["make", "-C", os.path.dirname(exe)], capture_output=True, text=True)
        if not os.path.exists(exe):
            flang = shutil.which("flang") or (os.path.exists("/opt/rocm/lib/llvm/bin/flang") and "/opt/rocm/lib/llvm/bin/flang")
            assert not flang, "Fortran host does not build although flang is present:\n" + r.stdout[-1500:] + r.stderr[-1500:]
            pytest.skip("no Fortran compiler on this box")
    for word in ("quietly", "hostX", "randomised_by_more_than_sixteen_characters", "Quiet", ""):
        r = subprocess.run([exe], cwd=str(tmp_path), env=dict(os.environ, PIC1DP_LOAD=word), capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "PIC1DP_LOAD must be host, random or quiet" in r.stdout + r.stderr, word
