"""The Fourier-Hermite spectrum of the markers (include/pic1dp_hip.h pic1dp_hip_hermite), the parts that need
no GPU: the terms on host arrays (pic1dp_hip_host_hermite) against tests/hermite_reference.py within the stated bound, the
recurrence's tables bit for bit, the orthonormality of the numpy recurrence, the pass plan at its boundaries (through the
probe library), the lengths and every refusal."""
import ctypes as C

import numpy as np
import pytest

import hermite_reference as HR


def host_markers(amd, inp, n):
    """the first n valid markers of the loader's block 0 of 1, on the host"""
    L = amd._lib.load()
    na, nv = C.c_int64(), C.c_int64()
    amd._lib.check(L.pic1dp_hip_block_sizes(C.byref(inp), 0, 0, 1, C.byref(na), C.byref(nv)))
    arrs = [np.empty(inp.nspecies * na.value) for _ in range(4)]
    amd._lib.check(L.pic1dp_hip_host_particle_load(C.byref(inp), 0, 1, *[a.ctypes.data_as(C.c_void_p) for a in arrs], na.value))
    assert nv.value >= n
    return [a[:n].copy() for a in arrs]


@pytest.fixture(scope="module")
def markers(amd):
    inp = amd.make_input(nparticle_max=2**12, nx=64)
    x, v, p, w = host_markers(amd, inp, 2**12)
    assert np.ptp(x) > 0.5 * inp.lx and np.any(w != 0.0) and np.ptp(v) > 4.0
    return inp, x, v, p, w


@pytest.fixture(scope="module")
def reference256(markers):
    """the reference at nherm 256, both sets, once: a smaller nherm is its first rows"""
    inp, x, v, p, w = markers
    return HR.reference(x, v, p, w, inp, modes=(0, 1, 5), nherm=256, v0=0.5, vt=1.25, which=3)


@pytest.mark.parametrize("nherm", [1, 2, 16, 17, 256])
@pytest.mark.parametrize("which", [1, 2, 3])
def test_host_hermite_against_the_reference(amd, markers, reference256, nherm, which):
    inp, x, v, p, w = markers
    got = amd.host_hermite(inp, x, v, p if which & 1 else None, w if which & 2 else None, modes=(0, 1, 5), nherm=nherm, v0=0.5,
                           vt=1.25, which=which)
    names = [n for bit, n in ((1, "total"), (2, "pertb")) if which & bit]
    assert got.shape == (len(names), 3, 2, nherm)
    for j, name in enumerate(names):
        full = reference256[name]
        ref = dict(exact=full["exact"][:, :, :nherm], abs=full["abs"][:, :, :nherm], count=full["count"])
        worst = HR.worst(got[j], ref, 0)             # (one sum in marker order: no partial sums are merged)
        print("host_hermite nherm %d which %d %s: worst error / bound = %.3g" % (nherm, which, name, worst))
        assert worst <= 1.0, (name, worst)
        assert not np.any(got[j][0, 1])              # mode 0: the sin row is exactly 0
        assert np.all(ref["abs"][1:] > 0) and np.any(got[j][1:] != 0.0)
    # n = 0, mode 0, cos: the sum of the weights
    assert abs(got[0][0, 0, 0] - np.sum(p if which & 1 else w)) <= 2**-40 * np.sum(np.abs(p if which & 1 else w))


def test_the_reference_is_the_definition_marker_by_marker(amd, markers):
    """host_hermite on ONE marker hands out single terms: the reference's terms bit for bit, up to the host's sincos against
    numpy's (a few ulp of the trig value)"""
    inp, x, v, p, w = markers
    for i in (0, 17, 4095):
        got = amd.host_hermite(inp, x[i:i + 1], v[i:i + 1], p[i:i + 1], w[i:i + 1], modes=(0, 1, 5), nherm=32, v0=0.5, vt=1.25)
        ref = HR.reference(x[i:i + 1], v[i:i + 1], p[i:i + 1], w[i:i + 1], inp, modes=(0, 1, 5), nherm=32, v0=0.5, vt=1.25)
        for j, name in enumerate(HR.SETS):
            assert np.all(np.abs(got[j] - ref[name]["exact"]) <= 8 * HR.U * ref[name]["abs"]), (i, name)
            assert np.array_equal(got[j][0, 0], ref[name]["exact"][0, 0])      # mode 0: cos(0) = 1 on both sides


def test_tables_are_numpys_bits(amd):
    for nherm in (1, 2, 255, 256):
        ra, rb = amd.hermite_tables(nherm)
        n1 = np.arange(1, nherm + 1, dtype=np.float64)
        assert np.array_equal(ra, 1.0 / np.sqrt(n1)) and np.array_equal(rb, np.sqrt(n1 - 1.0) / np.sqrt(n1))
        assert ra[0] == 1.0 and rb[0] == 0.0
    for bad in (0, 257, -1):
        with pytest.raises(amd.Pic1dpError) as ei:
            amd.hermite_tables(bad)
        assert ei.value.code == 1


def test_hermite_functions_are_orthonormal(amd):
    """300-point Gauss-Hermite rule (exact up to degree 599 > 2 * 127) with the weight exp(-u^2 / 2) / sqrt(2 pi)"""
    t, wt = np.polynomial.hermite_e.hermegauss(300)
    psi = amd.hermite_functions(t, 128)
    gram = (psi * (wt / np.sqrt(2.0 * np.pi))[None, :]) @ psi.T
    dev = float(np.max(np.abs(gram - np.eye(128))))
    print("hermite_functions: max |gram - 1| = %.3g" % dev)
    assert dev <= 1e-13
    assert np.array_equal(psi, HR.psi(t, 128))                   # the package's recurrence is the reference's
    assert amd.hermite_functions(np.zeros((2, 3)), 4).shape == (4, 2, 3)


def test_hermite_series_sums_the_functions(amd):
    v = np.linspace(-3.0, 4.0, 29)
    g = np.zeros(6, dtype=complex)
    g[0], g[3] = 2.0, 1.0 - 0.5j
    u = (v - 0.5) / 1.25
    he3 = (u**3 - 3.0 * u) / np.sqrt(6.0)
    want = (g[0] + g[3] * he3) * np.exp(-0.5 * u * u) / (np.sqrt(2.0 * np.pi) * 1.25)
    got = amd.hermite_series(g, v, v0=0.5, vt=1.25)
    assert got.shape == v.shape and np.allclose(got, want, rtol=1e-13, atol=1e-15)
    assert amd.hermite_series(np.stack([g, 2 * g]), v, 0.5, 1.25).shape == (2, 29)


def test_plan_at_its_boundaries(probe):
    P = probe.host_hermite_plan
    wave_lds = 8 * 2 * 16 * 66
    for nherm, nb in ((1, 4), (64, 4), (65, 8), (128, 8), (129, 16), (256, 16)):
        pl = P(nherm, 1, 2, 1, 10**6, 256)
        assert pl["nb"] == nb and pl["threads"] == 256 and pl["bytes"] == 4 * wave_lds
        assert 8 * 256 * nb <= pl["bytes"] <= 159 * 1024 and 2 * pl["bytes"] <= 160 * 1024
    # a workgroup per 4 waves x 16 trips x 64 markers, two per CU at most, one at least
    for n, blocks in ((0, 1), (1, 1), (4096, 1), (4097, 2), (8192, 2), (8193, 3), (512 * 4096, 512), (512 * 4096 + 1, 512), (10**8, 512)):
        pl = P(64, 4, 3, 1, n, 256)
        assert pl["blocks"] == blocks and pl["partials"] == blocks * 5, n
    assert P(64, 4, 3, 1, 10**8, 104)["blocks"] == 208
    # non-temporal loads beyond 288 MiB of the arrays read: 24 B a marker with one set, 32 B with both
    edge1, edge3 = 288 * 1048576 // 24, 288 * 1048576 // 32
    assert [P(64, 1, w, 1, edge1 + d, 256)["nt"] for w in (1, 2) for d in (0, 1)] == [0, 1, 0, 1]
    assert [P(64, 1, 3, 1, edge3 + d, 256)["nt"] for d in (0, 1)] == [0, 1]
    # no pass
    for args in ((0, 1, 1, 1), (257, 1, 1, 1), (64, 0, 1, 1), (64, 9, 1, 1), (64, 5, 3, 1), (64, 1, 0, 1), (64, 1, 4, 1), (64, 1, 2, 0), (64, 1, 3, 0)):
        assert P(*args, 1000, 256)["blocks"] == 0, args
    assert P(64, 8, 1, 0, 1000, 256)["blocks"] == 1 and P(64, 4, 3, 1, 1000, 256)["blocks"] == 1


def test_hermite_len(amd):
    assert amd.hermite_len((1,), 64, 3) == 2 * 1 * 2 * 64
    assert amd.hermite_len((0, 1, 2, 4), 100, 3) == 2 * 4 * 2 * 100
    assert amd.hermite_len(tuple(range(8)), 256, 1) == 8 * 2 * 256
    assert amd.hermite_len((3,), 1, 2) == 2


BAD = [dict(which=0), dict(which=4), dict(nherm=0), dict(nherm=257), dict(modes=()), dict(modes=tuple(range(9)), which=1),
       dict(modes=(0, 1, 2, 3, 4), which=3), dict(modes=(1, 1)), dict(modes=(-1,)), dict(vt=0.0), dict(vt=-1.0),
       dict(vt=float("inf")), dict(vt=float("nan")), dict(v0=float("inf")), dict(v0=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
def test_argument_errors(amd, markers, bad):
    inp, x, v, p, w = markers
    kw = dict(modes=(1,), nherm=8, v0=0.0, vt=1.0, which=3)
    kw.update(bad)
    with pytest.raises(amd.Pic1dpError) as ei:
        amd.host_hermite(inp, x[:4], v[:4], p[:4], w[:4], **kw)
    assert ei.value.code == 1
    with pytest.raises(amd.Pic1dpError) as ei:
        amd.hermite_len(kw["modes"], kw["nherm"], kw["which"], kw["v0"], kw["vt"])
    assert ei.value.code == 1


def test_argument_errors_that_need_the_input(amd, markers):
    inp, x, v, p, w = markers
    x, v, p, w = (a[:4] for a in (x, v, p, w))
    ok = amd.host_hermite(inp, x, v, p, w, modes=(inp.nx // 2,), nherm=4)
    assert ok.shape == (2, 1, 2, 4)
    L, lib = amd._lib.load(), amd._lib
    h = amd.make_hermite((1,), 4)
    out = np.full(16, 7.0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    full_f = amd.make_input(nparticle_max=2**12, nx=64, deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0])
    cases = [("mode beyond nx / 2", lambda: amd.host_hermite(inp, x, v, p, w, modes=(inp.nx // 2 + 1,), nherm=4)),
             ("species", lambda: amd.host_hermite(inp, x, v, p, w, nherm=4, ispecies=1)),
             ("species", lambda: amd.host_hermite(inp, x, v, p, w, nherm=4, ispecies=-1)),
             ("w of full f", lambda: amd.host_hermite(full_f, x, v, p, w, nherm=4, which=2)),
             ("w of full f", lambda: amd.host_hermite(full_f, x, v, p, w, nherm=4, which=3)),
             ("null p", lambda: amd.host_hermite(inp, x, v, None, w, nherm=4, which=3)),
             ("null w", lambda: amd.host_hermite(inp, x, v, p, None, nherm=4, which=2)),
             ("null input", lambda: lib.check(L.pic1dp_hip_host_hermite(None, 0, 3, C.byref(h), 4, ptr(x), ptr(v), ptr(p), ptr(w), ptr(out)))),
             ("null h", lambda: lib.check(L.pic1dp_hip_host_hermite(C.byref(inp), 0, 3, None, 4, ptr(x), ptr(v), ptr(p), ptr(w), ptr(out)))),
             ("null out", lambda: lib.check(L.pic1dp_hip_host_hermite(C.byref(inp), 0, 3, C.byref(h), 4, ptr(x), ptr(v), ptr(p), ptr(w), None))),
             ("negative np", lambda: lib.check(L.pic1dp_hip_host_hermite(C.byref(inp), 0, 3, C.byref(h), -1, ptr(x), ptr(v), ptr(p), ptr(w), ptr(out)))),
             ("null n", lambda: lib.check(L.pic1dp_hip_hermite_len(C.byref(h), 3, None))),
             ("null h", lambda: lib.check(L.pic1dp_hip_hermite_len(None, 3, C.byref(C.c_int64())))),
             ("null ra", lambda: lib.check(L.pic1dp_hip_hermite_tables(4, None, ptr(out))))]
    for what, call in cases:
        with pytest.raises(amd.Pic1dpError) as ei:
            call()
        assert ei.value.code == 1, what
    assert np.all(out == 7.0)                          # nothing was written
    assert amd.host_hermite(full_f, x, v, p, None, nherm=4, which=1).shape == (1, 1, 2, 4)
    assert not np.any(amd.host_hermite(inp, x[:0], v[:0], p[:0], w[:0], nherm=4))      # no marker: zeros
