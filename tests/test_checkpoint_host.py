"""The state digest and the checkpoint file on the host: no GPU.  tests/checkpoint_format.py restates both in numpy and
Python integers; the library's host_digest, checkpoint_info and checkpoint_verify are held against it, and
tests/checkpoint_check.cpp runs the library's writer and reader under the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import checkpoint_format as F
from conftest import ROOT

LENGTHS = (0, 1, 2, 63, 64, 65, 4095, 4096, 4097)


def crafted(n, seed=7):
    """n doubles: random bits, and -- as far as they fit -- +-0, +-inf, two NaN payloads, subnormals, equal values in
    different slots"""
    rng = np.random.default_rng(seed + n)
    a = rng.standard_normal(n)
    special = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000001,
                        0x7FF8000000000002, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x3FF8000000000000, 0x3FF8000000000000],
                       dtype=np.uint64).view(np.float64)
    k = min(n, special.size)
    a[:k] = special[:k]
    if n > 40:
        a[17] = a[33] = 2.5      # equal values in different slots
    return a


@pytest.mark.parametrize("n", LENGTHS)
def test_host_digest_equals_the_python_integers(amd, n):
    a = crafted(n)
    want = F.digest_int(a)
    assert amd.host_digest(a) == want
    assert F.digest(a) == want      # (the vectorised restatement the other tests use)
    if n == 0:
        assert want == 0


def test_host_digest_sees_position_and_every_bit(amd):
    a = crafted(65)
    base = amd.host_digest(a)
    # equal values in different slots count twice, each at its place: moving one of them elsewhere changes the word
    assert a[17] == a[33]
    b = a.copy()
    b[17], b[18] = a[18], a[17]
    assert amd.host_digest(b) != base
    # +0 / -0, and the two NaN payloads, differ
    assert amd.host_digest(np.array([0.0])) != amd.host_digest(np.array([-0.0]))
    nan = np.array([0x7FF8000000000001, 0x7FF8000000000002], dtype=np.uint64).view(np.float64)
    assert amd.host_digest(nan[:1]) != amd.host_digest(nan[1:])
    # swapping two unequal elements changes it, wherever they stand
    for i, j in ((0, 1), (2, 64), (30, 31)):
        b = a.copy()
        assert b[i:i + 1].tobytes() != b[j:j + 1].tobytes()
        b[i], b[j] = a[j], a[i]
        assert amd.host_digest(b) != base
    # flipping any single bit of any element changes it
    small = crafted(9)
    words = small.view(np.uint64)
    d0 = amd.host_digest(small)
    seen = set()
    for i in range(words.size):
        for bit in range(64):
            w = words.copy()
            w[i] ^= np.uint64(1 << bit)
            d = amd.host_digest(w.view(np.float64))
            assert d != d0 and d == F.digest_int(w.view(np.float64))
            seen.add(d)
    assert len(seen) == 64 * words.size


def make_state(amd, nalloc, np_valid, nhist, nblk=1, rng_words=5, seed=3, **kw):
    """a file's worth of state for the Python writer"""
    rng = np.random.default_rng(seed)
    ns = len(nalloc)
    inp = amd.make_input(nspecies=ns, nx=16, nmode=2, modes=[1, 2], nparticle_max=max(max(nalloc), 1), **kw)
    split = lambda n: [n // nblk + (1 if b < n % nblk else 0) for b in range(nblk)]   # noqa: E731
    return {
        "input": bytes(inp), "rank": 0, "nranks": 1, "npe": nblk, "nblk": nblk,
        "settings": dict(zip(F.SETTINGS, (1, 0, 1, 0, 1, 2, 5))), "rng_words": rng_words, "itime": 42, "rng_ready": 1 if rng_words else 0,
        "time": 4.2, "imerge": 1, "iremove": 2, "isplit": 3, "hist": rng.standard_normal(nhist),
        "nalloc": list(nalloc), "np": list(np_valid), "blk_np": [split(n) for n in np_valid],
        "markers": [{k: rng.standard_normal(n) for k in F.ARRAYS} for n in nalloc],
        "E": rng.standard_normal(16), "chargeden": rng.standard_normal(16), "mode_re": rng.standard_normal(2),
        "mode_im": rng.standard_normal(2),
        "rng": [{"engine": 3, "pos": 2 + b, "held": b & 1, "val": 0.25 * b, "q": rng.integers(0, 2**63, rng_words, dtype=np.uint64)}
                for b in range(nblk)],
        "fxb": rng.integers(0, 2**63, 4 * ns, dtype=np.uint64), "max_p": [1.5 + s for s in range(ns)],
        "max_w": [0.5 + s for s in range(ns)], "fixed": [s & 1 for s in range(ns)],
    }


CASES = {
    "one_species": dict(nalloc=[1000], np_valid=[1000], nhist=3),
    "two_species_unequal_np_below_nalloc": dict(nalloc=[1000, 777], np_valid=[900, 1], nhist=0, nblk=2),
    "empty_history_no_generators": dict(nalloc=[65], np_valid=[64], nhist=0, rng_words=0),
    "full_history": dict(nalloc=[4097], np_valid=[4000], nhist=1000),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_file_from_the_python_writer_is_accepted_and_described(amd, tmp_path, case):
    st = make_state(amd, **CASES[case])
    path = str(tmp_path / "ck.bin")
    F.write_file(path, st)
    amd.checkpoint_verify(path)
    info = amd.checkpoint_info(path)
    assert bytes(info["input"]) == st["input"]
    assert info["file_bytes"] == os.path.getsize(path) == F.sections(st)["total"][1]
    assert info["input_size"] == len(st["input"]) and info["format_version"] == F.VERSION
    for k in ("rank", "nranks", "npe", "nblk", "settings", "itime", "time", "imerge", "iremove", "isplit", "nalloc", "np"):
        assert info[k] == st[k], k
    assert info["rng_ready"] == bool(st["rng_ready"]) and info["hist_count"] == len(st["hist"])
    assert info["digest"] == [[F.digest_int(st["markers"][s][k]) for k in F.ARRAYS] for s in range(len(st["nalloc"]))]
    # ... and the Python reader takes its own file apart again
    back = F.parse_file(path, len(st["input"]), len(st["nalloc"]), 16, 2)
    assert back["settings"] == st["settings"] and np.array_equal(back["hist"], st["hist"])
    assert all(np.array_equal(back["markers"][s][k], st["markers"][s][k]) for s in range(len(st["nalloc"])) for k in F.ARRAYS)


def refused(amd, path, *words):
    for call in (amd.checkpoint_info, amd.checkpoint_verify):
        with pytest.raises(amd.Pic1dpError) as ei:
            call(path)
        assert ei.value.code == 1, str(ei.value)
        assert all(w in str(ei.value) for w in words), str(ei.value)


def test_malformed_files_are_refused_by_name(amd, tmp_path):
    st = make_state(amd, nalloc=[300, 200], np_valid=[300, 100], nhist=10, nblk=2)
    good = F.build(st)
    sec = F.sections(st)
    path = str(tmp_path / "bad.bin")

    def put(b):
        with open(path, "wb") as f:
            f.write(b)

    put(good)
    amd.checkpoint_verify(path)
    put(F.build(st, magic=b"PIC1DPXX"))
    refused(amd, path, "magic")
    put(F.build(st, version=F.VERSION + 1))
    refused(amd, path, "version %d" % (F.VERSION + 1))
    put(good[:-1])
    refused(amd, path, "truncated")
    put(good[:sec["digests"][0]])                     # the last section gone
    refused(amd, path, "truncated")
    put(good[:sec["markers1p"][0]] + good[sec["markers1p"][0] + sec["markers1p"][1]:])   # a marker section gone
    refused(amd, path, "truncated")
    put(good + b"\0")
    refused(amd, path, "1 more")
    put(F.build(st, input_size=len(st["input"]) + 8))
    refused(amd, path, "input struct of %d bytes" % (len(st["input"]) + 8))
    # one bit in a marker section: info has nothing against the file, verify names species and array
    for s, k in ((0, "x"), (1, "w"), (1, "p")):
        off = sec["markers%d%s" % (s, k)][0] + 8 * 57 + 3
        put(good[:off] + bytes([good[off] ^ 0x10]) + good[off + 1:])
        amd.checkpoint_info(path)
        with pytest.raises(amd.Pic1dpError) as ei:
            amd.checkpoint_verify(path)
        assert ei.value.code == 1 and "species %d, array %s" % (s, k) in str(ei.value), str(ei.value)
    # one bit in the field, history and generator sections (and the others the checksum covers)
    for name in ("fields", "history", "generators", "A", "fxb", "diag", "digests"):
        off = sec[name][0] + sec[name][1] // 2
        put(good[:off] + bytes([good[off] ^ 0x01]) + good[off + 1:])
        refused(amd, path, "checksum")
    with pytest.raises(amd.Pic1dpError) as ei:
        amd.checkpoint_info(str(tmp_path / "absent.bin"))
    assert "cannot open" in str(ei.value)


def test_writer_and_reader_under_the_host_sanitizers(tmp_path):
    """tests/checkpoint_check.cpp, a program of its own: checkpoint.cpp's Writer and Reader write, read and verify a small
    file, and the reader is fed the malformed files of the test above -- built with AddressSanitizer and
    UndefinedBehaviorSanitizer (host code only; nothing of it touches a GPU)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pic1dp_amd_build", os.path.join(ROOT, "pic1dp_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    exe = str(tmp_path / "checkpoint_check")
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "checkpoint_check.cpp"),
                           os.path.join(ROOT, "pic1dp_amd", "csrc", "checkpoint.cpp"), "-o", exe])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failed"), r.stdout


def test_info_struct_matches_the_header():
    """the ctypes mirror of pic1dp_checkpoint_info has the C struct's members in order"""
    from pic1dp_amd import _lib
    src = open(os.path.join(ROOT, "include", "pic1dp_hip.h")).read()
    body = src[src.index("typedef struct pic1dp_checkpoint_info {"):src.index("} pic1dp_checkpoint_info;")]
    import re
    names = re.findall(r"(\w+)(?:\[[^\]]*\])*(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in _lib.CheckpointInfo._fields_]
    assert C.sizeof(_lib.CheckpointInfo) % 8 == 0
