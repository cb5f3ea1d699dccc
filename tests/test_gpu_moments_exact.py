"""The exact velocity moments (include/pic1dp_hip.h pic1dp_hip_moments_exact) on the GPU against
tests/moments_exact.py, the definition in numpy and Python integers: limbs and doubles BIT FOR BIT.  Every case except the
overflow one first asserts that the definition itself sums every term of its inputs (a condition on the inputs).

Terms at the limit.  A term is summed when its ROUNDED count of quanta is below 2^44 in magnitude.  The largest value that
is summed is therefore one ulp below 2^44 - 1/2 quanta (it rounds to 2^44 - 1); 2^44 - 1/2 itself is a tie that goes to the
even 2^44 and is not summed, nor is any double from there to 2^44 and beyond.  The edge cases hold the summed side (one ulp
below the tie, and 2^44 - 1 itself), the overflow case the other side (the tie and 2^44): a case that asserts "no term is
rejected" cannot hold them."""
import ctypes as C
import math

import numpy as np
import pytest

import moments_exact as MX
import moments_reference as MR
import test_gpu_moments as G

pytestmark = pytest.mark.gpu

NAMES = ("total", "pertb")
MASK = (1 << 32) - 1


def context(amd, n_max, x, v, p, w, **kw):
    """a context of an input with nparticle_max = n_max (the quanta follow from it) holding exactly these markers"""
    e = amd.Pic1dp(amd.make_input(nparticle_max=max(n_max, 1), **kw))
    upload(e, x, v, p, w)
    return e


def upload(e, x, v, p, w):
    nalloc, _ = e.local_sizes()
    n = len(x)
    arrs = []
    for a in (x, v, p, w):
        full = np.zeros(nalloc)
        full[:n] = a
        arrs.append(full)
    e.particles_upload(*arrs, np_valid=n)


def check(e, x, v, p, w, which=3, what="", s=0):
    """limbs and doubles of context e against the definition on these markers, bit for bit"""
    ref = MX.reference(x, v, p, w, e.inp, which=which, ispecies=s)
    assert MX.in_range(ref), (what, ref["rejected"])
    limbs = e.moments_local_exact(s, which)
    assert limbs.dtype == np.int64 and limbs.shape == ref["limbs"].shape
    assert np.array_equal(limbs, ref["limbs"]), (what, np.argwhere(limbs != ref["limbs"])[:5])
    got = e.moments_exact(s, which)
    assert list(got) == list(ref["doubles"])
    for name in got:
        assert got[name].tobytes() == ref["doubles"][name].tobytes(), (what, name)
    return ref, limbs, got


def check_downloaded(e, which=3, what="", s=0):
    g = G.valid(e, s)
    return check(e, g["x"], g["v"], g["p"], g["w"], which, what, s)


def normalised(limbs):
    """the host's normalisation of element-wise sums: hi += lo >> 32, lo &= 2^32 - 1"""
    out = limbs.copy()
    out[:, :, 0, :] += limbs[:, :, 1, :] >> 32
    out[:, :, 1, :] = limbs[:, :, 1, :] & MASK
    return out


# ---------------------------------------------------------------------------
# 1. edges
# ---------------------------------------------------------------------------
def edge_markers(inp):
    nx, lx, vm = inp.nx, inp.lx, inp.v_max
    e = MX.quanta(inp)
    kb, kvm = e[0] + 40, MX.ceil_log2(vm)
    xs = G.edge_markers(lx, nx, vm)[0][::7]                    # the x list of test_gpu_moments.py::edge_markers
    assert xs.size == 11
    vs = [0.0, vm, -vm, 1.1, -2.7, 2.0 * vm, -2.0 * vm]
    qs = [1.5 * 2.0 ** (kb - 2), -2.25 * 2.0 ** (kb - 2), 0.0]  # scaled into range: |q| |v|^3 <= 18 2^(kb - 2) 2^(3 kvm) < 2^4 2^kb 2^(3 kvm)
    x, v, p, w = [], [], [], []
    for i, xi in enumerate(xs):
        for j, vj in enumerate(vs):
            x.append(xi), v.append(vj), p.append(qs[(i + j) % 3]), w.append(qs[(i + 2 * j + 1) % 3])
    # crafted from the definition: x = 0 has wl = 1 exactly, so a0 = q and b0 = 0; with v = 2^kvm every power holds
    # q 2^-e[0] quanta (e[k] = e[0] + k kvm), with v = 0 plane 0 alone
    top = math.nextafter(2.0 ** 44 - 0.5, 0.0)                  # one ulp below the tie that rounds to 2^44
    quanta = [2.0 ** 44 - 1.0, -(2.0 ** 44 - 1.0), top, -top, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 2.0 ** 43 + 0.5, 2.0 ** 43 + 1.5,
              -(2.0 ** 43 + 0.5), 2.0 ** 40 + 0.25, 2.0 ** 40 + 0.75]
    for i, m in enumerate(quanta):
        q = math.ldexp(m, e[0])
        assert math.ldexp(q, -e[0]) == m
        for vj in (2.0 ** kvm, 0.0):
            x.append(0.0), v.append(vj), p.append(q), w.append(math.ldexp(quanta[(i + 3) % len(quanta)], e[0]))
    return [np.array(a) for a in (x, v, p, w)], quanta


@pytest.mark.parametrize("nx", [2, 3, 8])
def test_edges(amd, nx):
    n = 77 + 30
    inp0 = amd.make_input(nparticle_max=n, nx=nx)
    (x, v, p, w), quanta = edge_markers(inp0)
    assert x.size == n
    e = context(amd, n, x, v, p, w, nx=nx)
    assert MX.quanta(e.inp) == MX.quanta(inp0) == amd.moments_quanta(e.inp)
    ref, _, _ = check(e, x, v, p, w, 3, "edges nx %d" % nx)
    for which in (1, 2):
        check(e, x, v, p, w, which, "edges nx %d which %d" % (nx, which))
    # the crafted terms are what they were crafted to be: a marker at x = 0 with v = 2^kvm holds round(m) quanta in all four planes
    singles = 0
    for i in range(n):                                           # every marker on its own
        upload(e, x[i:i + 1], v[i:i + 1], p[i:i + 1], w[i:i + 1])
        r1, l1, _ = check(e, x[i:i + 1], v[i:i + 1], p[i:i + 1], w[i:i + 1], 3, "edges nx %d marker %d" % (nx, i))
        singles += int(np.count_nonzero(l1))
        if i >= 77 and (i - 77) % 2 == 0:
            m = MX.quantise_py(quanta[(i - 77) // 2], 0)
            assert [r1["totals"][0][k][0] for k in range(4)] == [m] * 4, i
    assert singles > 100
    assert e.kernel_stats(18)[1] == 0


# ---------------------------------------------------------------------------
# 2. shapes of the sweep
# ---------------------------------------------------------------------------
N_SWEEP = 2**18 - 5


@pytest.fixture(scope="module")
def loader_markers(amd):
    """bump-on-tail markers from the loader, once"""
    e = G.loaded(amd, nparticle_max=N_SWEEP, nx=192)
    g = G.valid(e)
    e.close()
    return g


def dealt_trips(n, blocks, dyn_tail, block):
    """device_math.hpp pair_rows and k_moments_exact's cap of the drawn rows, for workgroup `block` of 1024 threads"""
    npair, stride, first = n >> 1, blocks * 1024, block * 1024
    dealt = -(-(npair - first) // stride) if first < npair else 0
    drawn = (dealt * dyn_tail) >> 4
    dealt -= drawn
    extra = drawn - 31
    return dealt + max(extra, 0)


@pytest.mark.parametrize("n", [0, 1, 2, 2047, 2049, 2**17 + 2**12 + 3, N_SWEEP])
def test_shapes_of_the_sweep(amd, probe, loader_markers, n):
    g = {k: a[:n] for k, a in loader_markers.items()}
    e = context(amd, n, g["x"], g["v"], g["p"], g["w"], nx=192)
    e.kernel_stats_enable(True)
    ref, limbs, got = check(e, g["x"], g["v"], g["p"], g["w"], 3, "np %d" % n)
    assert e.kernel_stats(17)[1] == (2 if n else 0)
    if n == 0:
        assert not np.any(limbs) and not np.any(got["total"]) and not np.any(got["pertb"])
    if n == N_SWEEP:
        # two workgroups, and in each at least 33 dealt trips: the flush inside the sweep (after trip 32) runs
        blocks = probe.host_moments_plan_exact(192, 3, 1, n, 256)["passes"][0]["blocks"]
        dyn_tail = probe.host_settings()["dyn_tail"]
        assert blocks == 2 and all(dealt_trips(n, blocks, dyn_tail, b) >= 33 for b in range(blocks))
        assert e.kernel_stats(17)[0] > 0.0


N_WINDOW = 2**17 + 2**12 + 3     # two workgroups of 34 and 33 rows


@pytest.fixture(scope="module")
def window_case(amd, loader_markers):
    """N_WINDOW markers, their definition and the limbs of a context at the default setting, once"""
    g = {k: a[:N_WINDOW] for k, a in loader_markers.items()}
    e = context(amd, N_WINDOW, g["x"], g["v"], g["p"], g["w"], nx=192)
    ref = MX.reference(g["x"], g["v"], g["p"], g["w"], e.inp, which=3)
    assert MX.in_range(ref)
    base = e.moments_local_exact(0, 3)
    e.close()
    return g, ref, base


@pytest.mark.parametrize("which", [1, 2, 3])
@pytest.mark.parametrize("drawn", ["0", "16"])
def test_rows_all_dealt_and_all_drawn_then_capped(amd, probe, monkeypatch, tuning, window_case, drawn, which):
    """tuning knob PIC1DP_DYN_TAIL at its two ends, the branches the shared sweep and window_rows (device_sweep.hpp) own: every
    row dealt -- the flush inside the sweep runs after trip 32 --, and every row drawn, of which the cap deals all but 31
    again.  The limbs are those of the default setting and of the definition, bit for bit"""
    g, ref, base = window_case
    blocks = probe.host_moments_plan_exact(192, which, 1, N_WINDOW, 256)["passes"][0]["blocks"]
    trips = [dealt_trips(N_WINDOW, blocks, int(drawn), b) for b in range(blocks)]
    assert blocks == 2 and trips == ([34, 33] if drawn == "0" else [3, 2])
    monkeypatch.setenv("PIC1DP_DYN_TAIL", drawn)
    e = context(amd, N_WINDOW, g["x"], g["v"], g["p"], g["w"], nx=192)
    limbs = e.moments_local_exact(0, which)
    sets = {1: slice(0, 1), 2: slice(1, 2), 3: slice(0, 2)}[which]
    assert np.array_equal(limbs, base[sets]), np.argwhere(limbs != base[sets])[:5]
    assert np.array_equal(limbs, ref["limbs"][sets]), np.argwhere(limbs != ref["limbs"][sets])[:5]
    assert e.kernel_stats(18)[1] == 0


# ---------------------------------------------------------------------------
# 3. one cell, one sign
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("signs", ["one_sign", "alternating_signs", "mixed_signs"])
def test_one_cell_carries_through_the_lo_limb(amd, signs):
    n, nx = 2**17 + 5, 8
    inp0 = amd.make_input(nparticle_max=n, nx=nx)
    e0 = MX.quanta(inp0)
    kvm = MX.ceil_log2(inp0.v_max)
    q = math.ldexp(2.0 ** 43, e0[0])                                 # 2^43 quanta in every plane with |v| = 2^kvm, x = 0
    i = np.arange(n)
    x = np.zeros(n)
    if signs == "one_sign":
        v, p = np.full(n, 2.0 ** kvm), np.full(n, q)
    elif signs == "alternating_signs":                               # -, +, -, ...: the total is -2^43, hi is negative
        v, p = np.full(n, 2.0 ** kvm), np.where(i % 2 == 0, -q, q)
    else:                                                            # two markers of three negative, so that the words a workgroup
                                                                     # flushes are negative too; v alternates: the odd powers differ
        v = np.where(i % 2 == 0, 2.0 ** kvm, -(2.0 ** kvm))
        p = np.where(i % 3 == 0, q, -q)
    w = -0.5 * p
    e = context(amd, n, x, v, p, w, nx=nx)
    ref, limbs, _ = check(e, x, v, p, w, 3, signs)
    if signs == "one_sign":
        assert ref["totals"][0][0][0] == n * 2**43 and limbs[0, 0, 0, 0] == (n * 2**43) >> 32          # ~2^60: far inside a word
        assert np.all(limbs[1, :, 0, 0] < 0)
    elif signs == "alternating_signs":
        assert ref["totals"][0][0][0] == -(2**43) and limbs[0, 0, 0, 0] == -(2**11) and limbs[0, 0, 1, 0] == 0
    else:
        assert ref["totals"][0][0][0] < 0 and limbs[0, 0, 0, 0] < 0 and limbs[0, 2, 0, 0] < 0
    assert np.all((limbs[:, :, 1, :] >= 0) & (limbs[:, :, 1, :] <= MASK))


# ---------------------------------------------------------------------------
# 4. order and split
# ---------------------------------------------------------------------------
def test_order_and_split_do_not_matter(amd, loader_markers):
    n, nx = 30_001, 192
    g = {k: a[:n] for k, a in loader_markers.items()}
    one = context(amd, n, g["x"], g["v"], g["p"], g["w"], nx=nx)
    ref, base, base_d = check(one, g["x"], g["v"], g["p"], g["w"], 3, "single context")
    perm = np.random.default_rng(3).permutation(n)
    upload(one, *(g[k][perm] for k in "xvpw"))
    assert np.array_equal(one.moments_local_exact(0, 3), base)
    one.close()
    for cuts in ([11_111], [7, 20_480]):
        total = np.zeros_like(base)
        lo, parts = 0, []
        for hi in cuts + [n]:
            parts.append(slice(lo, hi))
            lo = hi
        for sl in parts:
            e = context(amd, n, *(g[k][sl] for k in "xvpw"), nx=nx)
            local = e.moments_local_exact(0, 3)
            assert np.all((local[:, :, 1, :] >= 0) & (local[:, :, 1, :] <= MASK))
            total += local
            e.close()
        assert np.any(total[:, :, 1, :] > MASK)                      # (the element-wise sum is not normalised)
        assert np.array_equal(normalised(total), base), cuts
        conv = amd.moments_convert(one.inp, total, 3)
        for name in NAMES:
            assert conv[name].tobytes() == base_d[name].tobytes(), (cuts, name)


def test_two_ranks_equal_one_context_with_two_blocks(amd):
    kw = dict(nparticle_max=40_002, nx=64)
    one = amd.Pic1dp(amd.make_input(**kw), npe=2)
    one.particle_load()
    _, base, base_d = check_downloaded(one, 3, "npe 2")
    one.close()
    engs = [amd.Pic1dp(amd.make_input(**kw), rank=r, nranks=2, device=0) for r in range(2)]
    total = np.zeros_like(base)
    for e in engs:
        e.particle_load()
        _, local, _ = check_downloaded(e, 3, "rank %d" % e.rank)
        total += local
    assert np.array_equal(normalised(total), base)
    conv = amd.moments_convert(engs[0].inp, total, 3)
    for name in NAMES:
        assert conv[name].tobytes() == base_d[name].tobytes(), name


# ---------------------------------------------------------------------------
# 5. plan boundaries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nx,launches3,launches1", [(2400, 1, 1), (2401, 2, 1), (4800, 2, 1), (4801, 4, 2), (8192, 4, 2)])
def test_plan_boundaries(amd, nx, launches3, launches1):
    n = 5000
    rng = np.random.default_rng(nx)
    inp0 = amd.make_input(nparticle_max=n, nx=nx)
    kb = MX.quanta(inp0)[0] + 40
    x = rng.uniform(0.0, inp0.lx, n)
    v = np.clip(rng.normal(0.0, 2.0, n), -2.0 * inp0.v_max, 2.0 * inp0.v_max)
    p = rng.uniform(0.5, 1.0, n) * 2.0 ** kb
    w = np.clip(rng.normal(0.0, 0.1, n), -1.0, 1.0) * 2.0 ** kb
    e = context(amd, n, x, v, p, w, nx=nx)
    count = lambda: e.kernel_stats(17)[1]       # noqa: E731
    for which, launches in ((3, launches3), (1, launches1), (2, launches1)):
        ref = MX.reference(x, v, p, w, e.inp, which=which)
        assert MX.in_range(ref)
        c0 = count()
        limbs = e.moments_local_exact(0, which)
        assert count() - c0 == launches, (nx, which)
        assert np.array_equal(limbs, ref["limbs"]), (nx, which)
        got = e.moments_exact(0, which)
        for name in got:
            assert got[name].tobytes() == ref["doubles"][name].tobytes(), (nx, which, name)
    assert e.kernel_stats(16)[1] == 0


# ---------------------------------------------------------------------------
# 6. the non-temporal instance
# ---------------------------------------------------------------------------
def test_non_temporal_instance(amd, probe):
    n, nx = 9_500_000, 1024
    assert 32 * n > 288 * 1048576 and probe.host_moments_plan_exact(nx, 3, 1, n, 256)["passes"][0]["nt"] == 1
    e = G.loaded(amd, nparticle_max=n, nx=nx)
    g = G.valid(e)
    got = e.moments_exact(0, 3)
    ref = MX.reference(g["x"], g["v"], g["p"], g["w"], e.inp, which=3)
    assert MX.in_range(ref)
    for name in NAMES:
        assert got[name].tobytes() == ref["doubles"][name].tobytes(), name


# ---------------------------------------------------------------------------
# 7. against kind 0 and the unrounded sums
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(species_nparticle_init=[20000, 7001], **G.TWO)], ids=["deltaf", "deltaf_two_species"])
def test_against_the_fp64_moments_and_the_deposit(amd, kw):
    e = G.loaded(amd, nparticle_max=20000, nx=64, **kw)
    e.interaction_collect_charge()
    cd = e.get_field()["chargeden"]
    inp = e.inp
    charge = np.zeros(inp.nx)
    qbound = np.zeros(inp.nx)
    for s in range(inp.nspecies):
        g = G.valid(e, s)
        ref, _, got = check(e, g["x"], g["v"], g["p"], g["w"], 3, "species %d" % s, s)
        unrounded = MR.reference(g["x"], g["v"], g["p"], g["w"], inp, which=3)
        fp64 = e.moments(s, 3)
        nwg = MR.workgroups(g["x"].size)
        for name in NAMES:
            quant = ref["count"][None, :] * np.array([2.0 ** (ek - 1) for ek in ref["e"]])[:, None]
            err = np.abs(got[name] - unrounded[name]["exact"])
            print("exact moments, species %d %s: worst |exact - unrounded| / bound = %.3g" % (s, name, float(np.max(err / np.where(quant > 0, quant, 1.0)))))
            assert np.all(err <= quant), (s, name)
            err0 = np.abs(got[name] - fp64[name])
            tol0 = quant + MR.bound(unrounded[name], nwg)
            print("exact moments, species %d %s: worst |exact - moments()| / bound = %.3g" % (s, name, float(np.max(err0 / np.where(tol0 > 0, tol0, 1.0)))))
            assert np.all(err0 <= tol0), (s, name)
        z = inp.species_charge[s]
        charge = charge + got["pertb"][0] * z
        qbound = qbound + abs(z) * ref["count"] * 2.0 ** (ref["e"][0] - 1)
    mine = charge * float(inp.nx) / inp.lx
    scale = float(np.max(np.abs(cd)))
    tol = 2e-15 * scale + qbound * float(inp.nx) / inp.lx
    print("exact moments vs deposit: max |diff| / tolerance = %.3g" % float(np.max(np.abs(mine - cd) / tol)))
    assert scale > 0 and np.all(np.abs(mine - cd) <= tol)


def test_w_of_a_full_f_context_is_refused_by_name(amd):
    e = G.loaded(amd, nparticle_max=1000, nx=16, deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0])
    for call in (e.moments_exact, e.moments_local_exact):
        for which in (2, 3):
            with pytest.raises(amd.Pic1dpError) as ei:
                call(0, which)
            assert ei.value.code == 1 and "full-f" in str(ei.value) and "which = %d" % which in str(ei.value)
        for which in (0, 4):
            with pytest.raises(amd.Pic1dpError) as ei:
                call(0, which)
            assert ei.value.code == 1 and "which = %d" % which in str(ei.value)
        with pytest.raises(amd.Pic1dpError) as ei:
            call(1, 1)
        assert ei.value.code == 1 and "species" in str(ei.value)
    assert e.L.pic1dp_hip_moments_exact(e._ctx, 0, 1, None) == 1 and e.L.pic1dp_hip_moments_local_exact(e._ctx, 0, 1, None) == 1
    assert e.kernel_stats(17)[1] == 0
    check_downloaded(e, 1, "full f")
    fresh = amd.Pic1dp(amd.make_input(nparticle_max=100, nx=16))
    with pytest.raises(amd.Pic1dpError) as ei:
        fresh.moments_exact(0, 3)
    assert ei.value.code != 0 and "no particles" in str(ei.value)


# ---------------------------------------------------------------------------
# 8. overflow is loud and recoverable
# ---------------------------------------------------------------------------
def test_overflow_is_loud_and_recoverable(amd, loader_markers):
    n, nx = 3001, 64
    g = {k: a[:n].copy() for k, a in loader_markers.items()}
    good = {k: a.copy() for k, a in g.items()}
    g["v"][17] = 1e100
    g["p"][1234] = math.nan
    e = context(amd, n, g["x"], g["v"], g["p"], g["w"], nx=nx)
    e0 = MX.quanta(e.inp)
    ref = MX.reference(g["x"], g["v"], g["p"], g["w"], e.inp, which=3)
    assert ref["rejected"].tolist() == [[2, 4, 4, 4], [0, 2, 2, 2]]                 # (the NaN: set p, every power; 1e100: both sets from v^1 on)
    seen = e.kernel_stats(18)[1]
    assert seen == 0
    sentinel = 123.25
    for call, buf in ((e.L.pic1dp_hip_moments_exact, np.full((2, 4, nx), sentinel)),
                      (e.L.pic1dp_hip_moments_local_exact, np.full((2, 4, 2, nx), 77, dtype=np.int64))):
        keep = buf.copy()
        rc = call(e._ctx, 0, 3, buf.ctypes.data_as(C.c_void_p))
        msg = amd._lib.load().pic1dp_hip_last_error().decode()
        assert rc == 1, msg
        assert "2 term(s) of species 0, weight set p, power v^0" in msg and "2^%d" % e0[0] in msg, msg
        assert buf.tobytes() == keep.tobytes()                                     # nothing was handed out
        seen += int(ref["rejected"].sum())
        assert e.kernel_stats(18)[1] == seen
    # one weight set: w alone meets the 1e100 only
    with pytest.raises(amd.Pic1dpError) as ei:
        e.moments_exact(0, 2)
    assert ei.value.code == 1 and "2 term(s) of species 0, weight set w, power v^1" in str(ei.value)
    seen += 6
    assert e.kernel_stats(18)[1] == seen
    fp64 = e.moments(0, 3)                                                          # the FP64 kind still answers (non-finite bins and all)
    assert fp64["total"].shape == (4, nx) and not np.all(np.isfinite(fp64["total"]))
    # the other side of the limit: the tie 2^44 - 1/2 (rounds to the even 2^44) and 2^44 itself, in plane 0 alone (x = 0, v = 0)
    h = {k: a.copy() for k, a in good.items()}
    h["x"][5] = h["x"][6] = 0.0
    h["v"][5] = h["v"][6] = 0.0
    h["p"][5], h["w"][5] = math.ldexp(2.0 ** 44 - 0.5, e0[0]), -math.ldexp(2.0 ** 44, e0[0])
    h["p"][6], h["w"][6] = math.ldexp(math.nextafter(2.0 ** 44 - 0.5, 0.0), e0[0]), math.ldexp(2.0 ** 44 - 1.0, e0[0])
    upload(e, h["x"], h["v"], h["p"], h["w"])
    ref = MX.reference(h["x"], h["v"], h["p"], h["w"], e.inp, which=3)
    assert ref["rejected"].tolist() == [[1, 0, 0, 0], [1, 0, 0, 0]]
    with pytest.raises(amd.Pic1dpError) as ei:
        e.moments_local_exact(0, 3)
    assert ei.value.code == 1 and "1 term(s) of species 0, weight set p, power v^0" in str(ei.value)
    seen += 2
    assert e.kernel_stats(18)[1] == seen
    # in-range markers again: the call succeeds from zero counters, bit-equal to the definition
    upload(e, good["x"], good["v"], good["p"], good["w"])
    check(e, good["x"], good["v"], good["p"], good["w"], 3, "after the overflow")
    assert e.kernel_stats(18)[1] == seen


# ---------------------------------------------------------------------------
# 9. nothing changes between steps; inside a step the noted push is materialised
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,kw", [(2, dict()), (1, dict(nmode=2, modes=[1, 2]))], ids=["six_sums", "tiles_two_modes"])
def test_between_steps_nothing_changes(amd, monkeypatch, kind, kw):
    monkeypatch.setenv("PIC1DP_PREDICT", "1")
    monkeypatch.setenv("PIC1DP_PRED_KIND", str(kind))
    if kind == 2:
        monkeypatch.setenv("PIC1DP_FUSE_SOLVE", "2")
    a, b, c = (G.started(amd, nparticle_max=96, nx=32, **kw) for _ in range(3))
    for e in (a, b, c):
        assert e.predict_kind() == kind
        e.kernel_stats_enable(True)
        e.step(5)
    limbs, got = a.moments_local_exact(0, 3), a.moments_exact(0, 3)
    assert a.kernel_stats(17)[1] == 2 and b.kernel_stats(17)[1] == 0
    g = G.valid(c)                                # a third context's markers after the same five steps: the definition on them
    ref = MX.reference(g["x"], g["v"], g["p"], g["w"], c.inp, which=3)
    c.close()
    assert MX.in_range(ref) and np.any(limbs) and np.array_equal(limbs, ref["limbs"])
    for name in NAMES:
        assert got[name].tobytes() == ref["doubles"][name].tobytes(), name
    for e in (a, b):
        e.step(5)
    for e in (a, b):
        if kind == 2:
            assert e.kernel_stats(7)[1] == 8                                # all but the last step of each call
        assert e.kernel_stats(3)[1] == 1 and e.kernel_stats(6)[1] == 10    # one first-sub-step pass: the run's first step
    assert a.state_digest().tolist() == b.state_digest().tolist()
    fa, fb = a.get_field(), b.get_field()
    for k in ("electric", "chargeden", "mode_re", "mode_im"):
        assert fa[k].tobytes() == fb[k].tobytes(), k
    assert a.energy_history().tobytes() == b.energy_history().tobytes()
    assert a.get_field_half().tobytes() == b.get_field_half().tobytes()


def test_inside_a_step_lazy_and_eager_call_sites_give_the_same_limbs(amd, monkeypatch):
    kw = dict(nparticle_max=50_001, nx=96)
    monkeypatch.setenv("PIC1DP_PREDICT", "1")
    monkeypatch.setenv("PIC1DP_PRED_KIND", "2")
    a = G.started(amd, **kw)
    monkeypatch.setenv("PIC1DP_PREDICT", "0")
    monkeypatch.delenv("PIC1DP_PRED_KIND")
    monkeypatch.setenv("PIC1DP_LAZY_CALLS", "0")
    b = G.started(amd, **kw)
    monkeypatch.delenv("PIC1DP_LAZY_CALLS")
    b.set_electric(a.get_field()["electric"])
    for e in (a, b):
        e.kernel_stats_enable(True)
    for it in range(2):
        for irk in (1, 2):
            for e in (a, b):
                e.interaction_push_particle(irk)
            if irk == 1:
                # the lazy context has only noted its push: the call materialises it (a marker kernel runs); the eager one launches none
                before = [G.marker_launches(e) for e in (a, b)]
                la = a.moments_local_exact(0, 3)
                lb = b.moments_local_exact(0, 3)
                assert G.marker_launches(a) > before[0] and G.marker_launches(b) == before[1]
                assert np.array_equal(la, lb), it
                check_downloaded(b, 3, "eager, inside step %d" % it)
            for e in (a, b):
                e.interaction_collect_charge()
                e.field_solve_electric()
            fa, fb = a.get_field(), b.get_field()
            assert G.relerr(fa["electric"], fb["electric"]) < 1e-11, (it, irk)
            b.set_electric(fa["electric"])
        ga, gb = a.particles_download(), b.particles_download()
        for k in "xvw":
            assert np.array_equal(ga[k], gb[k]), (k, it)


# ---------------------------------------------------------------------------
# 10. after steps, on the GPU's own markers
# ---------------------------------------------------------------------------
def test_after_twenty_steps_of_the_default_case(amd):
    e = G.started(amd, nparticle_max=100_000)
    assert e.inp.nx == 192
    e.step(20)
    check_downloaded(e, 3, "after 20 steps")
    assert e.kernel_stats(18)[1] == 0
