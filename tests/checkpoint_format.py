"""The checkpoint file and the state digest (include/pic1dp_hip.h) restated in numpy and Python
integers, independently of the library: tests write files with write_file() for the library to read, and parse the library's
files with parse_file().

    header (64 B): magic "PIC1DPCK" | u32 version, u32 0x01020304 | u64 total bytes | u64 sizeof(pic1dp_input) | u64 checksum
                   | u64 bytes of header + section A | u64 bytes of the tail | u64 0
    section A    : the input struct (padded to 8) | i32 rank, nranks, npe, nblk | i32 settings[7], i32 rng_words
                   | i32 itime, i32 rng_ready, f64 time | i32 imerge, iremove, isplit, 0 | i64 history count
                   | per species: i64 nalloc, i64 np, i64 blk_np[nblk]
    markers      : per species x, v, w, p, nalloc doubles each, in logical order
    tail         : E[nx], chargeden[nx], mode_re[nmode], mode_im[nmode] | history | per block (rng_words > 0): i32 engine,
                   pos, held, 0, f64 spare, u64 q[rng_words] | per species u64 fxb[4] | per species f64 max_p, max_w, i32
                   fixed, 0 | per species u64 D[4]
The checksum is the digest's sum over the 8-byte words of header (checksum word zero), section A and tail, in file order.
"""
import struct

import numpy as np

MASK = (1 << 64) - 1
GOLD, M1, M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
MAGIC = b"PIC1DPCK"
VERSION = 1
ENDIAN = 0x01020304
HEADER = 64
SETTINGS = ("charge_sum", "diag_sum", "field_transform", "field_solver", "step_mode", "fuse_output", "seed_offset")
ARRAYS = "xvwp"


def mix(u, i):
    """the word of slot i holding the 64 bits u (Python integers)"""
    z = (u + (i + 1) * GOLD) & MASK
    z = ((z ^ (z >> 30)) * M1) & MASK
    z = ((z ^ (z >> 27)) * M2) & MASK
    return z ^ (z >> 31)


def digest_int(a):
    """D of an array of doubles, in Python integers (slow: small arrays)"""
    words = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    return sum(mix(int(u), i) for i, u in enumerate(words)) & MASK


def digest_words(words, i0=0):
    """the same sum over uint64 words standing at slots i0, i0 + 1, ..., in numpy's wrapping uint64 arithmetic"""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = w + (np.arange(i0 + 1, i0 + 1 + w.size, dtype=np.uint64) * np.uint64(GOLD))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(M2)
        z = z ^ (z >> np.uint64(31))
        return int(np.sum(z, dtype=np.uint64))


def digest(a):
    return digest_words(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64))


def _pad8(b):
    return b + b"\0" * (-len(b) % 8)


def _f64(a):
    return np.ascontiguousarray(a, dtype="<f8").tobytes()


def build(st, version=VERSION, magic=MAGIC, input_size=None):
    """the bytes of a file holding the state st (a dict: see parse_file)"""
    ns, nblk = len(st["nalloc"]), st["nblk"]
    a = _pad8(bytes(st["input"]))
    a += struct.pack("<4i", st["rank"], st["nranks"], st["npe"], nblk)
    a += struct.pack("<8i", *[st["settings"][n] for n in SETTINGS], st["rng_words"])
    a += struct.pack("<2id", st["itime"], st["rng_ready"], st["time"])
    a += struct.pack("<4i", st["imerge"], st["iremove"], st["isplit"], 0)
    a += struct.pack("<q", len(st["hist"]))
    for s in range(ns):
        a += struct.pack("<2q", st["nalloc"][s], st["np"][s]) + struct.pack("<%dq" % nblk, *st["blk_np"][s])
    markers = b"".join(_f64(st["markers"][s][k]) for s in range(ns) for k in ARRAYS)
    for s in range(ns):
        assert all(len(st["markers"][s][k]) == st["nalloc"][s] for k in ARRAYS)
    t = _f64(st["E"]) + _f64(st["chargeden"]) + _f64(st["mode_re"]) + _f64(st["mode_im"]) + _f64(st["hist"])
    if st["rng_words"] > 0:
        for r in st["rng"]:
            t += struct.pack("<4id", r["engine"], r["pos"], r["held"], 0, r["val"])
            t += np.ascontiguousarray(r["q"], dtype="<u8").tobytes()
    t += np.ascontiguousarray(st["fxb"], dtype="<u8").tobytes()
    for s in range(ns):
        t += struct.pack("<2d2i", st["max_p"][s], st["max_w"][s], st["fixed"][s], 0)
    dig = st.get("digest") or [[digest(st["markers"][s][k]) for k in ARRAYS] for s in range(ns)]
    for s in range(ns):
        t += struct.pack("<4Q", *dig[s])
    head_bytes = HEADER + len(a)
    total = head_bytes + len(markers) + len(t)
    isz = len(bytes(st["input"])) if input_size is None else input_size

    def header(checksum):
        return magic + struct.pack("<2I6Q", version, ENDIAN, total, isz, checksum, head_bytes, len(t), 0)
    small = header(0) + a + t
    return header(digest_words(np.frombuffer(small, dtype="<u8"))) + a + markers + t


def write_file(path, st, **kw):
    with open(path, "wb") as f:
        f.write(build(st, **kw))


def sections(st):
    """name -> (offset, length) of every section of the file build(st) gives"""
    ns, nblk = len(st["nalloc"]), st["nblk"]
    out, at = {"header": (0, HEADER)}, HEADER
    alen = len(_pad8(bytes(st["input"]))) + 16 + 32 + 16 + 16 + 8 + ns * (16 + 8 * nblk)
    out["A"] = (at, alen)
    at += alen
    for s in range(ns):
        for k in ARRAYS:
            out["markers%d%s" % (s, k)] = (at, 8 * st["nalloc"][s])
            at += 8 * st["nalloc"][s]
    nx, nm = len(st["E"]), len(st["mode_re"])
    for name, n in (("fields", 16 * nx + 16 * nm), ("history", 8 * len(st["hist"])),
                    ("generators", nblk * (24 + 8 * st["rng_words"]) if st["rng_words"] > 0 else 0),
                    ("fxb", 32 * ns), ("diag", 24 * ns), ("digests", 32 * ns)):
        out[name] = (at, n)
        at += n
    out["total"] = (0, at)
    return out


def parse_file(path, input_size, nspecies, nx, nmode):
    """the state a file holds, as the dict build() takes (input: its raw bytes); checksum and digests are verified"""
    b = open(path, "rb").read()
    assert b[:8] == MAGIC
    version, endian, total, isz, checksum, head_bytes, tail_bytes, zero = struct.unpack_from("<2I6Q", b, 8)
    assert (version, endian, total, isz, zero) == (VERSION, ENDIAN, len(b), input_size, 0)
    st, at = {"input": b[HEADER:HEADER + input_size]}, HEADER + len(_pad8(b"\0" * input_size))
    st["rank"], st["nranks"], st["npe"], st["nblk"] = struct.unpack_from("<4i", b, at)
    vals = struct.unpack_from("<8i", b, at + 16)
    st["settings"], st["rng_words"] = dict(zip(SETTINGS, vals[:7])), vals[7]
    st["itime"], st["rng_ready"], st["time"] = struct.unpack_from("<2id", b, at + 48)
    st["imerge"], st["iremove"], st["isplit"], _ = struct.unpack_from("<4i", b, at + 64)
    nhist, = struct.unpack_from("<q", b, at + 80)
    at += 88
    nblk = st["nblk"]
    st["nalloc"], st["np"], st["blk_np"] = [], [], []
    for s in range(nspecies):
        na, npv = struct.unpack_from("<2q", b, at)
        st["nalloc"].append(na), st["np"].append(npv)
        st["blk_np"].append(list(struct.unpack_from("<%dq" % nblk, b, at + 16)))
        at += 16 + 8 * nblk
    assert at == head_bytes

    def f64(n):
        nonlocal at
        a = np.frombuffer(b, dtype="<f8", count=n, offset=at).copy()
        at += 8 * n
        return a
    st["markers"] = [{k: f64(st["nalloc"][s]) for k in ARRAYS} for s in range(nspecies)]
    tail_off = at
    st["E"], st["chargeden"], st["mode_re"], st["mode_im"], st["hist"] = f64(nx), f64(nx), f64(nmode), f64(nmode), f64(nhist)
    st["rng"] = []
    if st["rng_words"] > 0:
        for _ in range(nblk):
            engine, pos, held, _z, val = struct.unpack_from("<4id", b, at)
            at += 24
            q = np.frombuffer(b, dtype="<u8", count=st["rng_words"], offset=at).copy()
            at += 8 * st["rng_words"]
            st["rng"].append({"engine": engine, "pos": pos, "held": held, "val": val, "q": q})
    st["fxb"] = np.frombuffer(b, dtype="<u8", count=4 * nspecies, offset=at).copy()
    at += 32 * nspecies
    st["max_p"], st["max_w"], st["fixed"] = [], [], []
    for s in range(nspecies):
        mp, mw, fx, _z = struct.unpack_from("<2d2i", b, at)
        st["max_p"].append(mp), st["max_w"].append(mw), st["fixed"].append(fx)
        at += 24
    st["digest"] = [list(struct.unpack_from("<4Q", b, at + 32 * s)) for s in range(nspecies)]
    at += 32 * nspecies
    assert at == len(b) and at - tail_off == tail_bytes
    small = b[:32] + b"\0" * 8 + b[40:head_bytes] + b[tail_off:]
    assert digest_words(np.frombuffer(small, dtype="<u8")) == checksum
    for s in range(nspecies):
        assert st["digest"][s] == [digest(st["markers"][s][k]) for k in ARRAYS]
    return st
