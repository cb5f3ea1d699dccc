"""The exact wave-particle power (include/pic1dp_hip.h pic1dp_hip_power_exact) on the GPU against
tests/power_exact.py, the definition in numpy and Python integers: limbs, the call's exponent and the doubles BIT FOR BIT.
Every case that expects a result first asserts that the definition itself sums every term of its inputs (a condition on
the inputs).  The helpers and the planted markers are tests/test_gpu_power.py's."""
import ctypes as C
import math

import numpy as np
import pytest

import power_exact as PX
import power_reference as PR
import test_gpu_power as G

pytestmark = pytest.mark.gpu

NAMES = ("total", "pertb")
MASK = (1 << 32) - 1
FULL_F = dict(deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0])
TWO = dict(nspecies=2, species_charge=[-1.0, 2.0], species_mass=[1.0, 4.0], species_temperature=[1.0, 0.5],
           species_temperature2=[1.0, 0.5], species_density=[0.9, 0.9], species_v0=[5.0, 5.0])


def sets_of(which):
    return {1: slice(0, 1), 2: slice(1, 2), 3: slice(0, 2)}[which]


def upload(e, x, v, p, w, junk=None, s=0):
    nalloc, _ = e.local_sizes(s)
    n = len(x)
    arrs = []
    for k, a in enumerate((x, v, p, w)):
        full = np.zeros(nalloc) if junk is None else np.full(nalloc, junk[k])
        full[:n] = a
        arrs.append(full)
    e.particles_upload(*arrs, ispecies=s, np_valid=n)


def check(e, E, which=3, what="", s=0, markers=None, ref=None):
    """limbs, exponent and doubles of context e against the definition on its markers (or those given) and the field E"""
    import pic1dp_amd as amd
    if ref is None:
        g = G.valid(e, s) if markers is None else markers
        ref = PX.reference(g["x"], g["v"], g["p"], g["w"], E, e.inp, which=which, ispecies=s)
    assert PX.in_range(ref), (what, ref["rejected"])
    limbs, eq = e.power_local_exact(s, which)
    assert limbs.dtype == np.int64 and limbs.shape == ref["limbs"].shape
    assert eq == ref["e"] == amd.power_quantum(e.inp, float(np.max(np.abs(E))), s), (what, eq, ref["e"])
    assert np.array_equal(limbs, ref["limbs"]), (what, np.argwhere(limbs != ref["limbs"])[:5])
    got = e.power_exact(s, which)
    conv = amd.power_convert(e.inp, ref["limbs"], ref["e"], which)
    assert list(got) == list(ref["doubles"]) == list(conv)
    for name in got:
        for key in ("xv", "v"):
            assert got[name][key].tobytes() == conv[name][key].tobytes() == ref["doubles"][name][key].tobytes(), (what, name, key)
        assert got[name]["rest"] == conv[name]["rest"] == ref["doubles"][name]["rest"], (what, name)
    return ref, limbs, got


def normalised(limbs, nxv):
    """the host's normalisation of element-wise sums: hi += lo >> 32, lo &= 2^32 - 1 (planes and the rest pair)"""
    out = limbs.copy()
    out[:, :nxv] += limbs[:, nxv:2 * nxv] >> 32
    out[:, nxv:2 * nxv] = limbs[:, nxv:2 * nxv] & MASK
    out[:, 2 * nxv] += limbs[:, 2 * nxv + 1] >> 32
    out[:, 2 * nxv + 1] = limbs[:, 2 * nxv + 1] & MASK
    return out


# ---------------------------------------------------------------------------
# 1. edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), FULL_F], ids=["deltaf", "full_f"])
@pytest.mark.parametrize("nx,nxo,nvo", [(2, 1, 2), (3, 3, 5), (8, 64, 64)])
def test_edges(amd, nx, nxo, nvo, kw):
    """(2, 1, 2): one x cell and two v rows whose top row keeps the marker -- four terms of a marker in one word"""
    inp0 = amd.make_input(nparticle_max=1, nx=nx, nx_opd=nxo, nv_opd=nvo, **kw)
    x, v, p, w = G.edge_markers(inp0.lx, nx, inp0.v_max)
    assert np.max(np.abs(p)) <= 2.25 and np.max(np.abs(w)) <= 2.25
    E = G.random_field(nx, 100 + nx)
    e = amd.Pic1dp(amd.make_input(nparticle_max=x.size + 29, nx=nx, nx_opd=nxo, nv_opd=nvo, **kw))
    upload(e, x, v, p, w, junk=(3.3, -4.4, 7.0, -9.0))
    assert e.local_sizes()[0] > x.size == e.local_sizes()[1]     # (junk in the tail slots)
    e.set_electric(E)
    g = dict(x=x, v=v, p=p, w=w)
    for which in ((1, 2, 3) if not kw else (1,)):
        ref, limbs, got = check(e, E, which, "edges nx %d %d x %d which %d" % (nx, nxo, nvo, which), markers=g)
        assert np.any(limbs[:, :nxo * nvo] | limbs[:, nxo * nvo:2 * nxo * nvo]) and np.any(limbs[:, -2:])
        for name in got:
            assert ref["rest_count"][name] == 5 * 4
    if nxo == 1:
        top = nvo - 1                                            # v just below v_max: c00 = c01 = c10 = c11
        assert ref["count"]["total"][top, 0] >= 4 * 5 and int(ref["count"]["total"].sum()) == 4 * 15
    assert e.power_exact_stats()[2] == 0
    # every marker on its own (slot 0; the others are tail slots now)
    nalloc, _ = e.local_sizes()
    for i in range(x.size):
        arrs = [np.roll(np.concatenate([a, np.zeros(nalloc - a.size)]), -i) for a in (x, v, p, w)]
        e.particles_upload(*arrs, np_valid=1)
        check(e, E, 1 if kw else 3, "marker %d alone" % i, markers={k: a[i:i + 1] for k, a in g.items()})


# ---------------------------------------------------------------------------
# 2. order and shape
# ---------------------------------------------------------------------------
N_ORDER = 200_001


@pytest.fixture(scope="module")
def loader_markers(amd):
    """bump-on-tail markers from the loader, once.  The loader keeps |v| < v_max = 8; the contexts that take these markers have
    v_max = 4, so that some of them have no bins and feed rest"""
    e = G.loaded(amd, nparticle_max=2**18, nx=64)
    assert e.inp.v_max == 8.0
    g = G.valid(e)
    e.close()
    assert g["x"].size == 2**18 and np.count_nonzero(np.abs(g["v"][:3000]) >= 4.0) > 3
    return g


@pytest.fixture(scope="module")
def order_case(amd, loader_markers):
    """N_ORDER markers at nx 64, 64 x 64, their field and definition, once"""
    g = {k: a[:N_ORDER] for k, a in loader_markers.items()}
    E = G.random_field(64, 7)
    inp = amd.make_input(nparticle_max=N_ORDER, nx=64, v_max=4.0)
    ref = PX.reference(g["x"], g["v"], g["p"], g["w"], E, inp, which=3)
    assert PX.in_range(ref) and min(ref["rest_count"].values()) > 100
    return g, E, ref


def test_order_and_launch_shape_do_not_matter(amd, order_case):
    g, E, ref = order_case
    e = G.uploaded(amd, g["x"], g["v"], g["p"], g["w"], nx=64, v_max=4.0)
    assert (e.inp.nx_opd, e.inp.nv_opd) == (64, 64)
    e.set_electric(E)
    _, base, base_d = check(e, E, 3, "np %d" % N_ORDER, ref=ref)
    for which in (1, 2):
        assert np.array_equal(e.power_local_exact(0, which)[0], base[sets_of(which)])
    for shape in ((64, 1), (256, 2), (1024, 1)):
        e.set_launch(*shape)
        limbs, eq = e.power_local_exact(0, 3)
        assert np.array_equal(limbs, base) and eq == ref["e"], shape
    e.set_launch(0, 0)
    perm = np.random.default_rng(3).permutation(N_ORDER)
    upload(e, *(g[k][perm] for k in "xvpw"))
    limbs, eq = e.power_local_exact(0, 3)
    assert np.array_equal(limbs, base) and eq == ref["e"]
    got = e.power_exact(0, 3)
    for name in NAMES:
        assert got[name]["xv"].tobytes() == base_d[name]["xv"].tobytes() and got[name]["v"].tobytes() == base_d[name]["v"].tobytes()
        assert got[name]["rest"] == base_d[name]["rest"]


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_few_markers(amd, loader_markers, n):
    far = np.flatnonzero(np.abs(loader_markers["v"][:3000]) >= 4.0)[:1]
    idx = np.concatenate([far, np.arange(8)])[:n]              # (the first of them has no bins)
    g = {k: a[idx] for k, a in loader_markers.items()}
    e = G.uploaded(amd, g["x"], g["v"], g["p"], g["w"], junk=(1.0, 2.0, 3.0, 4.0), nx=64, v_max=4.0)
    E = G.random_field(64, 9)
    e.set_electric(E)
    c0 = e.power_exact_stats()[1]
    ref, limbs, got = check(e, E, 3, "np %d" % n, markers=g)
    assert e.power_exact_stats()[1] - c0 == (2 if n else 0)      # (local_exact and exact: one pass each)
    if n == 0:
        assert not np.any(limbs)
        for name in NAMES:
            assert not np.any(got[name]["xv"]) and not np.any(got[name]["v"]) and got[name]["rest"] == 0.0
    else:
        assert np.any(limbs[:, -2:])


# ---------------------------------------------------------------------------
# 3. rank split
# ---------------------------------------------------------------------------
def test_two_halves_add_up_to_the_whole_bit_for_bit(amd, order_case):
    g, E, _ = order_case
    n = 60_001
    gs = {k: a[:n] for k, a in g.items()}
    whole = G.uploaded(amd, gs["x"], gs["v"], gs["p"], gs["w"], nx=64, v_max=4.0)
    whole.set_electric(E)
    wref, base, base_d = check(whole, E, 3, "the whole", markers=gs)
    nxv = 64 * 64
    total = np.zeros_like(base)
    for sl in (slice(0, 30_000), slice(30_000, n)):
        e = amd.Pic1dp(amd.make_input(nparticle_max=n, nx=64, v_max=4.0))      # (the whole's input: the whole's quantum)
        upload(e, *(gs[k][sl] for k in "xvpw"))
        e.set_electric(E)
        local, eq = e.power_local_exact(0, 3)
        assert eq == wref["e"]
        assert np.all((local[:, nxv:2 * nxv] >= 0) & (local[:, nxv:2 * nxv] <= MASK)) and np.all((local[:, -1] >= 0) & (local[:, -1] <= MASK))
        total += local
        e.close()
    assert np.any(total[:, nxv:2 * nxv] > MASK)                      # (the element-wise sum is not normalised)
    assert np.array_equal(normalised(total, nxv), base)
    conv = amd.power_convert(whole.inp, total, wref["e"], 3)
    for name in NAMES:
        assert conv[name]["xv"].tobytes() == base_d[name]["xv"].tobytes() and conv[name]["v"].tobytes() == base_d[name]["v"].tobytes()
        assert conv[name]["rest"] == base_d[name]["rest"]


# ---------------------------------------------------------------------------
# 4. windows
# ---------------------------------------------------------------------------
def dealt_trips(n, blocks, dyn_tail, block):
    """device_math.hpp pair_rows and window_rows' cap of the drawn rows, for workgroup `block` of 1024 threads"""
    npair, stride, first = n >> 1, blocks * 1024, block * 1024
    dealt = -(-(npair - first) // stride) if first < npair else 0
    drawn = (dealt * dyn_tail) >> 4
    dealt -= drawn
    return dealt + max(drawn - 31, 0)


@pytest.mark.parametrize("n", [2**17, 2**17 + 1, 2**18 - 5])
def test_windows(amd, probe, loader_markers, n):
    """2^17 markers are 64 rows of one workgroup: the flush inside the sweep runs (after 32 dealt trips) and the words go on
    from zero.  2^17 + 1 markers are two workgroups by the plan's rule, with the odd last marker before the sweep; 2^18 - 5
    puts the odd marker and a flush inside the sweep into the same workgroups"""
    g = {k: a[:n] for k, a in loader_markers.items()}
    blocks = probe.host_power_plan_exact(64, 64, 64, 3, 1, n, 256)["passes"][0]["blocks"]
    dyn_tail = probe.host_settings()["dyn_tail"]
    trips = [dealt_trips(n, blocks, dyn_tail, b) for b in range(blocks)]
    assert blocks == (1 if n == 2**17 else 2)
    if n != 2**17 + 1:
        assert min(trips) >= 33, trips
    e = G.uploaded(amd, g["x"], g["v"], g["p"], g["w"], nx=64, v_max=4.0)
    E = G.random_field(64, 11)
    e.set_electric(E)
    ref, limbs, _ = check(e, E, 3, "np %d" % n, markers=g)
    assert min(ref["rest_count"].values()) > 100 and np.any(limbs[:, -2:], axis=1).all()
    assert e.power_exact_stats()[2] == 0


# ---------------------------------------------------------------------------
# 5. every branch of the plan
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nxo,nvo,launches", [(1024, 64, 64, 1), (8192, 96, 96, 2), (64, 160, 160, 1)],
                         ids=["one_pass", "pass_per_set", "straight"])
def test_every_branch_of_the_plan(amd, probe, nx, nxo, nvo, launches):
    n = 200_000
    rng = np.random.default_rng(2017)
    u, v, p, w = rng.uniform(0.0, 1.0, n), rng.normal(0.0, 2.2, n), rng.uniform(0.5, 1.5, n), rng.normal(0.0, 0.1, n)
    inp0 = amd.make_input(nparticle_max=n, nx=nx, nx_opd=nxo, nv_opd=nvo, v_max=4.0)
    x = u * inp0.lx
    scale = 2.0 ** (amd.charge_quantum(inp0, 0) + 52 - 1)       # the weights within the input's bound 2^kb (exact scaling)
    p, w = p * scale, w * scale
    assert np.count_nonzero(np.abs(v) >= inp0.v_max) > 100
    plan =probe.host_power_plan_exact(nx, nxo, nvo, 3, 1, n, 256)
    assert len(plan["passes"]) == launches and plan["passes"][0]["lds"] == (0 if nxo == 160 else 1) and plan["passes"][0]["blocks"] == 2
    e = G.uploaded(amd, x, v, p, w, nx=nx, nx_opd=nxo, nv_opd=nvo, v_max=4.0)
    E = G.random_field(nx, nx + nxo)
    e.set_electric(E)
    g = dict(x=x, v=v, p=p, w=w)
    ref = PX.reference(x, v, p, w, E, e.inp, which=3)
    assert PX.in_range(ref)
    e.kernel_stats_enable(True)
    c0 = e.power_exact_stats()[1]
    limbs, eq = e.power_local_exact(0, 3)
    assert e.power_exact_stats()[1] - c0 == launches and e.power_exact_stats()[0] > 0.0
    assert eq == ref["e"] and np.array_equal(limbs, ref["limbs"]), np.argwhere(limbs != ref["limbs"])[:5]
    for which in (1, 2):
        c0 = e.power_exact_stats()[1]
        one, _ = e.power_local_exact(0, which)
        assert e.power_exact_stats()[1] - c0 == 1
        assert np.array_equal(one, ref["limbs"][sets_of(which)]), which
    check(e, E, 3, "nx %d %d x %d" % (nx, nxo, nvo), markers=g, ref=ref)


# ---------------------------------------------------------------------------
# 6. the scale follows the field
# ---------------------------------------------------------------------------
def field_with_max(nx, top, seed):
    """a field whose max |E| is exactly `top`, met at one cell with a minus sign"""
    E = np.random.default_rng(seed).uniform(-0.9, 0.9, nx) * top
    E[nx // 3] = -top
    assert float(np.max(np.abs(E))) == top
    return E


@pytest.fixture(scope="module")
def scale_context(amd, loader_markers):
    n = 5001
    g = {k: a[:n] for k, a in loader_markers.items()}
    e = G.uploaded(amd, g["x"], g["v"], g["p"], g["w"], nx=64, v_max=4.0)
    yield e, g
    e.close()


@pytest.mark.parametrize("top", [2.0, math.nextafter(2.0, 3.0), math.nextafter(2.0, 0.0), 2.0 ** -30, 1e-300, 0.0],
                         ids=["2", "2_up", "2_down", "2^-30", "1e-300", "zeros"])
def test_scale(amd, scale_context, top):
    e, g = scale_context
    E = field_with_max(64, top, 5) if top else np.zeros(64)
    e.set_electric(E)
    ref, limbs, got = check(e, E, 3, "max |E| %r" % top, markers=g)
    kb, kvm = amd.charge_quantum(e.inp, 0) + 52, 2
    kE = {2.0: 1, math.nextafter(2.0, 3.0): 2, math.nextafter(2.0, 0.0): 1, 2.0 ** -30: -30, 1e-300: -996, 0.0: 0}[top]
    assert ref["e"] == max(kb + kvm + kE - 40, -1000) == amd.power_quantum(e.inp, top)
    if top == 0.0:
        assert not np.any(limbs)
        for name in NAMES:
            assert not np.any(got[name]["xv"]) and got[name]["rest"] == 0.0
    elif top == 1e-300:                                              # the clamp: a quantum of 2^-1000, a few quanta per term at most
        assert ref["e"] == -1000
    else:
        assert np.any(limbs)


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf], ids=["nan", "inf", "minus_inf"])
@pytest.mark.parametrize("n", [5001, 0])
def test_a_field_that_is_not_finite_is_refused(amd, loader_markers, bad, n):
    g = {k: a[:n] for k, a in loader_markers.items()}
    e = G.uploaded(amd, g["x"], g["v"], g["p"], g["w"], nx=64, v_max=4.0)
    E = G.random_field(64, 3)
    e.set_electric(E)
    check(e, E, 3, "before", markers=g)
    bad_E = E.copy()
    bad_E[41] = bad
    e.set_electric(bad_E)
    c23, c24 = e.power_exact_stats()[1], e.power_exact_stats()[2]
    L = amd._lib.load()
    out = np.full(2 * (64 * 64 + 64 + 1), 123.25)
    limbs = np.full(2 * (2 * 64 * 64 + 2), 77, dtype=np.int64)
    eq = C.c_int32(-12345)
    for call in (lambda: L.pic1dp_hip_power_exact(e._ctx, 0, 3, out.ctypes.data_as(C.c_void_p)),
                 lambda: L.pic1dp_hip_power_local_exact(e._ctx, 0, 3, limbs.ctypes.data_as(C.c_void_p), C.byref(eq))):
        rc = call()
        msg = L.pic1dp_hip_last_error().decode()
        assert rc == 1 and "field not finite" in msg, msg
    assert np.all(out == 123.25) and np.all(limbs == 77) and eq.value == -12345
    assert e.power_exact_stats()[1] == c23 and e.power_exact_stats()[2] == c24
    e.set_electric(E)                                               # a finite field again: the call answers
    check(e, E, 3, "after", markers=g)


# ---------------------------------------------------------------------------
# 7. out of range
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["bins", "rest", "nan"])
def test_out_of_range_is_loud_and_recoverable(amd, loader_markers, case):
    n, k = 3001, 1234
    good = {key: a[:n].copy() for key, a in loader_markers.items()}
    far = int(np.flatnonzero(np.abs(good["v"]) >= 4.0)[0])
    assert abs(good["v"][k]) < 4.0
    e = G.uploaded(amd, good["x"], good["v"], good["p"], good["w"], nx=64, v_max=4.0)
    E = np.full(64, 2.0)                                             # e = 2 at every marker, kE = 1
    e.set_electric(E)
    kb = amd.charge_quantum(e.inp, 0) + 52
    g = {key: a.copy() for key, a in good.items()}
    if case == "bins":                                               # |p| = 64 B_s on a grid point of x, v = v_max / 2
        g["x"][k], g["v"][k], g["p"][k] = 0.0, 2.0, -64.0 * 2.0 ** kb
        want, which_sets = "weight set p, bins", (3, 1)
    elif case == "rest":                                             # |v| = 64 v_max: no bins
        g["v"][far], g["w"][far], g["p"][far] = 256.0, 2.0 ** kb, 0.0
        want, which_sets = "weight set w, rest", (3, 2)
    else:
        g["p"][k] = math.nan
        want, which_sets = "weight set p, bins", (3, 1)
    upload(e, g["x"], g["v"], g["p"], g["w"])
    ref = PX.reference(g["x"], g["v"], g["p"], g["w"], E, e.inp, which=3)
    j, col = (1, 1) if case == "rest" else (0, 0)
    count = int(ref["rejected"][j, col])
    assert count >= 1 and int(ref["rejected"].sum()) == count and (case != "nan" or count == 4)
    seen = e.power_exact_stats()[2]
    passes = e.power_exact_stats()[1]
    L = amd._lib.load()
    for which in which_sets:
        nsets = 2 if which == 3 else 1
        out = np.full(nsets * (64 * 64 + 64 + 1), 123.25)
        limbs = np.full(nsets * (2 * 64 * 64 + 2), 77, dtype=np.int64)
        eq = C.c_int32(-12345)
        for call in (lambda: L.pic1dp_hip_power_exact(e._ctx, 0, which, out.ctypes.data_as(C.c_void_p)),
                     lambda: L.pic1dp_hip_power_local_exact(e._ctx, 0, which, limbs.ctypes.data_as(C.c_void_p), C.byref(eq))):
            rc = call()
            msg = L.pic1dp_hip_last_error().decode()
            assert rc == 1, msg
            assert "%d term(s) of species 0, %s" % (count, want) in msg and "2^%d" % ref["e"] in msg, msg
            seen += count
            passes += 1
            assert e.power_exact_stats()[2] == seen and e.power_exact_stats()[1] == passes
        assert np.all(out == 123.25) and np.all(limbs == 77) and eq.value == -12345          # nothing was handed out
    other = 2 if case != "rest" else 1                               # the other weight set alone does not meet the marker
    one, _ = e.power_local_exact(0, other)
    assert np.array_equal(one, ref["limbs"][sets_of(other)]) and e.power_exact_stats()[2] == seen
    fp64 = e.power(0, 3)                                             # the FP64 kind still answers
    assert fp64["total"]["xv"].shape == (64, 64)
    upload(e, good["x"], good["v"], good["p"], good["w"])            # the marker fixed: zero counters, the definition
    check(e, E, 3, "after the fix", markers=good)
    assert e.power_exact_stats()[2] == seen


# ---------------------------------------------------------------------------
# 8. against the real sum, and kind 0 beside it
# ---------------------------------------------------------------------------
def test_against_the_real_sum_and_kind_0(amd, loader_markers):
    """per bin |power_exact - fsum(terms)| <= n_b 2^(e - 1) + 2^-53 |total|: half a quantum per term, one conversion"""
    n = 40_001
    g = {k: a[:n] for k, a in loader_markers.items()}
    e = G.uploaded(amd, g["x"], g["v"], g["p"], g["w"], nx=64, v_max=4.0)
    E = G.random_field(64, 13)
    e.set_electric(E)
    xref = PX.reference(g["x"], g["v"], g["p"], g["w"], E, e.inp, which=3)
    assert PX.in_range(xref)
    real = PR.reference(g["x"], g["v"], g["p"], g["w"], E, e.inp, which=3)
    got = e.power_exact(0, 3)
    kind0 = e.power(0, 3)
    half = math.ldexp(1.0, xref["e"] - 1)
    for name in NAMES:
        r = real[name]
        b = r["count"] * half + PR.U * np.abs(r["exact"])
        err = np.abs(got[name]["xv"] - r["exact"])
        print("power_exact %s: worst error / bound = %.3g" % (name, G.ratio(err, b)))
        assert np.all(err <= b), name
        br = r["rest"]["count"] * half + PR.U * abs(r["rest"]["exact"])
        assert r["rest"]["count"] > 10 and abs(got[name]["rest"] - r["rest"]["exact"]) <= br, name
        rows = np.array([math.fsum(row) for row in r["exact"].tolist()])
        bv = r["count"].sum(axis=1) * half + PR.U * np.abs(rows) + 64 * PR.U * np.abs(r["exact"]).sum(axis=1)   # (the rows of rounded fsums)
        assert np.all(np.abs(got[name]["v"] - rows) <= bv), name
        G.within(kind0[name], r, PR.workgroups(n), "kind 0 %s" % name)


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
    (limbs, eq), got = a.power_local_exact(0, 3), a.power_exact(0, 3)
    assert a.power_exact_stats()[1] == 2 and b.power_exact_stats()[1] == 0
    g = G.valid(c)                                # a third context's markers and field after the same five steps
    E = c.get_field()["electric"]
    ref = PX.reference(g["x"], g["v"], g["p"], g["w"], E, c.inp, which=3)
    c.close()
    assert PX.in_range(ref) and np.any(limbs) and np.array_equal(limbs, ref["limbs"]) and eq == ref["e"]
    for name in NAMES:
        assert got[name]["xv"].tobytes() == ref["doubles"][name]["xv"].tobytes(), name
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
                la, ea = a.power_local_exact(0, 3)
                lb, eb = b.power_local_exact(0, 3)
                assert G.marker_launches(a) > before[0] and G.marker_launches(b) == before[1]
                assert np.array_equal(la, lb) and ea == eb, it
                check(b, b.get_field()["electric"], 3, "eager, inside step %d" % it)
            for e in (a, b):
                e.interaction_collect_charge()
                e.field_solve_electric()
            fa, fb = a.get_field(), b.get_field()
            assert np.max(np.abs(fa["electric"] - fb["electric"])) <= 1e-11 * np.max(np.abs(fb["electric"])), (it, irk)
            b.set_electric(fa["electric"])
        ga, gb = a.particles_download(), b.particles_download()
        for k in "xvw":
            assert np.array_equal(ga[k], gb[k]), (k, it)


# ---------------------------------------------------------------------------
# 10. two species; refusals
# ---------------------------------------------------------------------------
def test_two_species_each_against_the_definition(amd):
    e = G.started(amd, nparticle_max=20_000, nx=64, species_nparticle_init=[20_000, 7_001], **TWO)
    e.step(3)
    E = e.get_field()["electric"]
    assert np.any(E)
    for s in range(2):
        _, limbs, _ = check(e, E, 3, "species %d" % s, s=s)
        assert np.any(limbs)
    assert e.power_exact_stats()[2] == 0


def test_refusals_name_the_cause(amd):
    e = G.loaded(amd, nparticle_max=1000, nx=16, **FULL_F)
    for call in (e.power_exact, e.power_local_exact):
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
    L = amd._lib.load()
    assert L.pic1dp_hip_power_exact(e._ctx, 0, 1, None) == 1 and b"null output" in L.pic1dp_hip_last_error()
    limbs = np.zeros(2 * 64 * 64 + 2, dtype=np.int64)
    assert L.pic1dp_hip_power_local_exact(e._ctx, 0, 1, limbs.ctypes.data_as(C.c_void_p), None) == 1 and b"null output" in L.pic1dp_hip_last_error()
    assert L.pic1dp_hip_power_local_exact(e._ctx, 0, 1, None, C.byref(C.c_int32())) == 1 and b"null output" in L.pic1dp_hip_last_error()
    assert e.power_exact_stats()[1] == 0
    assert list(e.power_exact(0, 1)) == ["total"] and e.power_exact_stats()[1] == 1
    fresh = amd.Pic1dp(amd.make_input(nparticle_max=1000, nx=16))
    with pytest.raises(amd.Pic1dpError) as ei:
        fresh.power_exact(0, 1)
    assert ei.value.code != 0 and "no particles" in str(ei.value)
