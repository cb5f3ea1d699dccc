"""The exact phase-space histogram on a caller's window and grid (include/pic1dp_hip.h pic1dp_hip_zoom) on the
GPU against tests/zoom_reference.py, the rule in numpy and Python integers on the context's own download: the limbs BIT FOR
BIT, then the doubles.  There is no tolerance anywhere.  Contexts that hold crafted markers have tail slots filled with junk
that lies INSIDE every window used here, so a kernel that reads the tail shows."""
import ctypes as C
import math

import numpy as np
import pytest

import test_gpu_power as G
import zoom_reference as Z

pytestmark = pytest.mark.gpu

TAIL = 5
NMAX = 2**17 + 4097
FULL_F = dict(deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0])
WHICH = {1: [0], 2: [1], 4: [2], 7: [0, 1, 2], 5: [0, 2], 3: [0, 1], 6: [1, 2]}       # the planes of a mask, as rows of which = 7


def quanta(amd, inp, s=0):
    e = amd.diag_quanta(inp, s)
    return e[1], e[2]


def uploaded(amd, x, v, p, w, tail=TAIL, **kw):
    """a context holding exactly these markers as its valid ones; the tail slots hold junk inside every window used here"""
    n = len(x)
    kw.setdefault("nx", 16)
    e = amd.Pic1dp(amd.make_input(nparticle_max=n + tail, **kw))
    upload(e, x, v, p, w)
    assert e.local_sizes()[0] >= n + tail
    return e


def upload(e, x, v, p, w):
    nalloc, n = e.local_sizes()[0], len(x)
    arrs = []
    for a, junk in zip((x, v, p, w), (1.5, 3.5, -7.0, -9.0)):       # (x 1.5, v 3.5: inside every window below)
        full = np.full(nalloc, junk)
        full[:n] = a
        arrs.append(full)
    e.particles_upload(*arrs, np_valid=n)


def check(amd, e, xw, vw, bins, ref=None, masks=(7, 1, 2, 4), what=""):
    """limbs and doubles of context e against the rule on its own download, for every mask (the planes are independent: a
    mask's reference is rows of which = 7's)"""
    if ref is None:
        g = G.valid(e)
        ref = Z.reference(g["x"], g["v"], g["p"], g["w"], e.inp.lx, xw, vw, bins, 7, *quanta(amd, e.inp))
    assert ref["rejected"] == [0, 0, 0], what
    for which in masks:
        rows = WHICH[which]
        limbs = e.zoom_local_exact(0, x=xw, v=vw, bins=bins, which=which)
        part = dict(limbs=ref["limbs"][rows])
        assert limbs.dtype == np.int64
        Z.assert_same(limbs, part, "%s which %d" % (what, which))
        got = e.zoom(0, x=xw, v=vw, bins=bins, which=which)
        conv = amd.zoom_convert(e.inp, limbs, x=xw, v=vw, bins=bins, which=which)
        names = [Z.PLANES[k] for k in rows]
        assert list(got)[:len(names)] == names
        for j, name in zip(rows, names):
            assert got[name].tobytes() == conv[name].tobytes() == ref["doubles"][j].tobytes(), (what, which, name)
    return ref


@pytest.fixture(scope="module")
def loader_markers(amd):
    """bump-on-tail markers from the loader, once; |v| < v_max = 8"""
    e = G.loaded(amd, nparticle_max=NMAX, nx=64)
    g = G.valid(e)
    e.close()
    assert g["x"].size == NMAX
    return g


def dealt_trips(n, blocks, dyn_tail, block):
    """device_math.hpp pair_rows and window_rows' cap of the drawn rows, for workgroup `block` of 1024 threads"""
    npair, stride, first = n >> 1, blocks * 1024, block * 1024
    dealt = -(-(npair - first) // stride) if first < npair else 0
    drawn = (dealt * dyn_tail) >> 4
    dealt -= drawn
    return dealt + max(drawn - 31, 0)


def past_the_cap(probe, np_):
    """(nxb, nvb) of the smallest 160-column grid of three planes the plan sends to memory"""
    cap = probe.host_zoom_plan(64, 64, 7, 1, np_, 256)["pass_cap"]
    nvb = 40 * cap + 1                                       # 19 200 / (3 x 160) = 40 rows a pass
    assert [ps["lds"] for ps in probe.host_zoom_plan(160, nvb, 7, 1, np_, 256)["passes"]] == [0]
    assert [ps["lds"] for ps in probe.host_zoom_plan(160, nvb - 1, 7, 1, np_, 256)["passes"]] == [1] * cap
    return 160, nvb


# ---------------------------------------------------------------------------
# 1. marker counts x grids x masks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4097, 100_001, 2**17, NMAX])
def test_marker_counts_and_grids(amd, probe, loader_markers, n):
    """100 001 markers are one workgroup of 49 trips, but with the library's drawn tail (dyn_tail 8: half the rows are drawn)
    only 25 of them are dealt, so the flush INSIDE the sweep (after 32 dealt trips) does not run there -- computed from the
    plan below, not assumed.  2^17 markers are the one-workgroup size at which it does (33 dealt trips); 2^17 + 4097 are
    two workgroups."""
    g = {k: a[:n] for k, a in loader_markers.items()}
    e = uploaded(amd, g["x"], g["v"], g["p"], g["w"], nx=64)
    lx = e.inp.lx
    try:
        plan = probe.host_zoom_plan(64, 64, 7, 1, n, 256)
        assert [ps["lds"] for ps in plan["passes"]] == [1] and plan["passes"][0]["bytes"] == 8 * 12288       # 64 x 64 x 3 fits
        blocks = plan["passes"][0]["blocks"]
        assert blocks == (2 if n == NMAX else 1)
        trips = [dealt_trips(n, blocks, probe.host_settings()["dyn_tail"], b) for b in range(blocks)]
        if n == 2**17:         # one workgroup whose flush inside the sweep runs: more than 32 dealt trips
            assert trips[0] >= 33, trips
        else:
            assert max(trips) < 32, trips
        banded = probe.host_zoom_plan(160, 160, 7, 1, n, 256)["passes"]
        assert len(banded) > 1 and all(ps["lds"] for ps in banded) and sum(ps["rows"] for ps in banded) == 160
        whole, vall = (0.0, lx), (-8.0, 8.0)
        before = e.zoom_stats()[1]
        for bins in ((1, 1), (1, 64), (64, 1), (64, 64), (160, 160), past_the_cap(probe, n)):
            ref = check(amd, e, whole, vall, bins, what="n %d %s" % (n, bins))
            assert ref["inside"] == n == sum(ref["totals"][0])                      # every loader marker lies in the whole box
        assert e.zoom_stats()[1] > before and e.zoom_stats()[2] == 0
        check(amd, e, (0.9 * lx, 0.2 * lx), (3.0, 5.0), (160, 160), what="n %d straddling" % n)
        check(amd, e, (0.25 * lx, 0.5 * lx), (-1.0, 6.5), (64, 64), masks=(7, 5, 3, 6), what="n %d window" % n)
    finally:
        e.close()


# ---------------------------------------------------------------------------
# 2. nothing to do
# ---------------------------------------------------------------------------
def test_the_empty_window_launches_nothing_and_an_unpopulated_one_gives_zeros(amd, loader_markers):
    n = 4097
    g = {k: a[:n] for k, a in loader_markers.items()}
    e = uploaded(amd, g["x"], g["v"], g["p"], g["w"], nx=64)
    try:
        e.kernel_stats_enable(True)
        passes = e.zoom_stats()[1]
        for bins in ((64, 64), (160, 160)):
            limbs = e.zoom_local_exact(0, x=(2.0, 2.0), v=(-8.0, 8.0), bins=bins)
            assert limbs.shape == (3, 2, bins[1], bins[0]) and not np.any(limbs)
            assert not np.any(e.zoom(0, x=(2.0, 2.0), v=(-8.0, 8.0), bins=bins)["markr"])
        assert e.zoom_stats()[1] == passes                                          # x_lo == x_hi: no marker was read
        limbs = e.zoom_local_exact(0, x=(1.0, 3.0), v=(20.0, 30.0), bins=(64, 64))   # a window no marker lies in
        assert not np.any(limbs) and e.zoom_stats()[1] == passes + 1
        ms, n_pass, rej = e.zoom_stats()
        assert ms > 0.0 and rej == 0
    finally:
        e.close()


# ---------------------------------------------------------------------------
# 3. planted markers, every edge
# ---------------------------------------------------------------------------
PLANTED = [((0.0, None), (-8.0, 8.0), (64, 64)), ((1.0, 3.0), (3.0, 5.0), (7, 5)), ((15.0, 2.0), (-1.5, 4.25), (5, 3)),
           ((None, 3.0), (-2.0, 4.0), (3, 4)), (Z.CLAMP_X["x"], (-1.0, 4.0), (Z.CLAMP_X["nxb"], 3)),
           ((1.0, 3.0), Z.CLAMP_V["v"], (3, Z.CLAMP_V["nvb"])), ((1.0, 3.0), (3.0, 5.0), (160, 160))]


@pytest.mark.parametrize("xw,vw,bins", PLANTED)
def test_planted_markers(amd, xw, vw, bins):
    lx = amd.make_input(nparticle_max=1, nx=16).lx
    xw = tuple(lx if t is None else t for t in xw)
    n = Z.planted(lx, xw, vw, 0, 0)[0].size
    inp = amd.make_input(nparticle_max=n + TAIL, nx=16)                             # the context's input: its quanta
    x, v, p, w = Z.planted(inp.lx, xw, vw, *quanta(amd, inp))
    e = uploaded(amd, x, v, p, w)
    assert quanta(amd, e.inp) == quanta(amd, inp) and len(x) == n
    try:
        inside, _, _ = Z.cells(np.array([1.5]), np.array([3.5]), inp.lx, xw, vw, bins)
        assert inside[0]                                                             # the tail's junk lies in the window
        g = G.valid(e)
        for k, a in zip("xvpw", (x, v, p, w)):
            assert g[k].tobytes() == a.tobytes()                                     # the download is what was planted
        ref = check(amd, e, xw, vw, bins, what="planted %s" % (bins,))
        assert ref["inside"] >= 10 and ref["inside"] == e.select_count(0, x=xw, v=vw)
    finally:
        e.close()


# ---------------------------------------------------------------------------
# 4. anchors and invariances
# ---------------------------------------------------------------------------
def test_anchors_and_invariances(amd, probe, loader_markers):
    n = 60_001
    g = {k: a[:n] for k, a in loader_markers.items()}
    e = uploaded(amd, g["x"], g["v"], g["p"], g["w"], nx=64)
    lx = e.inp.lx
    cases = [((0.9 * lx, 0.2 * lx), (3.0, 5.0), (64, 64)), ((0.0, lx), (-8.0, 8.0), (160, 160)), ((1.0, 9.0), (-2.0, 2.0), past_the_cap(probe, n))]
    try:
        base = []
        for xw, vw, bins in cases:
            limbs = e.zoom_local_exact(0, x=xw, v=vw, bins=bins)
            total = int(limbs[0, 0].sum()) * 2**32 + int(limbs[0, 1].sum())
            assert total == e.select_count(0, x=xw, v=vw) > 100                      # the window is select's
            base.append(limbs)
        for threads, bpc in ((1024, 1), (192, 3), (64, 24), (512, 2)):               # set_launch shapes
            e.set_launch(threads, bpc)
            for (xw, vw, bins), want in zip(cases, base):
                assert np.array_equal(e.zoom_local_exact(0, x=xw, v=vw, bins=bins), want), (threads, bpc, bins)
        e.set_launch(0, 0)
        perm = np.random.default_rng(4).permutation(n)                               # the order of the markers
        upload(e, *(g[k][perm] for k in "xvpw"))
        for (xw, vw, bins), want in zip(cases, base):
            assert np.array_equal(e.zoom_local_exact(0, x=xw, v=vw, bins=bins), want), bins
    finally:
        e.close()


def test_two_ranks_add_up_to_one_context_bit_for_bit(amd):
    kw = dict(nparticle_max=3 * 4096 + 5, nx=64)
    one = amd.Pic1dp(amd.make_input(**kw))
    two = [amd.Pic1dp(amd.make_input(**kw), rank=r, nranks=2) for r in range(2)]
    try:
        for e in [one] + two:
            e.particle_load_device(1)
        assert sum(e.local_sizes()[1] for e in two) == one.local_sizes()[1]
        lx = one.inp.lx
        for xw, vw, bins in (((0.8 * lx, 0.4 * lx), (-3.0, 6.0), (64, 64)), ((0.0, lx), (-8.0, 8.0), (160, 160))):
            kwz = dict(x=xw, v=vw, bins=bins)
            whole = one.zoom_local_exact(0, **kwz)
            parts = [e.zoom_local_exact(0, **kwz) for e in two]
            total = parts[0] + parts[1]
            assert np.any(total[:, 1] >= 2**32)                                      # (the element-wise sum is not normalised)
            norm = total.copy()
            norm[:, 0] += total[:, 1] >> 32
            norm[:, 1] = total[:, 1] & (2**32 - 1)
            assert np.array_equal(norm, whole)
            conv, got = amd.zoom_convert(one.inp, total, **kwz), one.zoom(0, **kwz)
            for name in Z.PLANES:
                assert conv[name].tobytes() == got[name].tobytes(), name
            check(amd, one, xw, vw, bins, masks=(7,), what="one context")
    finally:
        for e in [one] + two:
            e.close()


# ---------------------------------------------------------------------------
# 5. terms that are not summed; refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [(64, 64), (160, 160), "memory"])
def test_a_rejected_term_is_loud_and_recoverable(amd, probe, loader_markers, bins):
    n, k = 3001, 1234
    bins = past_the_cap(probe, n) if bins == "memory" else bins
    good = {key: a[:n].copy() for key, a in loader_markers.items()}
    e = uploaded(amd, good["x"], good["v"], good["p"], good["w"], nx=64)
    lx = e.inp.lx
    xw, vw = (0.0, lx), (-8.0, 8.0)
    e_p, e_w = quanta(amd, e.inp)
    try:
        g = {key: a.copy() for key, a in good.items()}
        g["p"][k], g["p"][k + 1], g["w"][k + 5] = math.ldexp(1.0, e_p + 44), math.nan, -math.inf
        upload(e, g["x"], g["v"], g["p"], g["w"])
        ref = Z.reference(g["x"], g["v"], g["p"], g["w"], lx, xw, vw, bins, 7, e_p, e_w)
        assert ref["rejected"] == [0, 2, 1]
        _, passes, seen = e.zoom_stats()
        L = amd._lib.load()
        z = amd.make_zoom(e.inp, xw, vw, bins)
        cells = bins[0] * bins[1]
        for which, plane, count, e_q in ((7, "total", 2, e_p), (2, "total", 2, e_p), (4, "pertb", 1, e_w), (5, "pertb", 1, e_w)):
            nplanes = len(WHICH[which])
            out = np.full(nplanes * cells, 123.25)
            limbs = np.full(2 * nplanes * cells, 77, dtype=np.int64)
            for call in (lambda: L.pic1dp_hip_zoom(e._ctx, 0, C.byref(z), which, out.ctypes.data_as(C.c_void_p)),
                         lambda: L.pic1dp_hip_zoom_local_exact(e._ctx, 0, C.byref(z), which, limbs.ctypes.data_as(C.c_void_p))):
                rc = call()
                msg = L.pic1dp_hip_last_error().decode()
                assert rc == 1, msg
                assert "%d term(s) of species 0, plane %s" % (count, plane) in msg and "2^%d" % e_q in msg, msg
                seen += sum(ref["rejected"][j] for j in WHICH[which])
                assert e.zoom_stats()[2] == seen
            assert np.all(out == 123.25) and np.all(limbs == 77)                     # nothing was handed out
        assert e.zoom_stats()[1] > passes
        markr = e.zoom_local_exact(0, x=xw, v=vw, bins=bins, which=1)               # each plane judges its own term: markr answers
        assert np.array_equal(markr, ref["limbs"][[0]]) and int(markr[0, 1].sum()) == n and e.zoom_stats()[2] == seen
        upload(e, good["x"], good["v"], good["p"], good["w"])                       # the markers fixed: zero counters, the definition
        check(amd, e, xw, vw, bins, masks=(7,), what="after the fix")
        assert e.zoom_stats()[2] == seen
    finally:
        e.close()


def test_refusals_with_a_context(amd):
    e = G.loaded(amd, nparticle_max=1000, nx=16, **FULL_F)
    try:
        for which in (4, 5, 6, 7):
            with pytest.raises(amd.Pic1dpError) as ei:
                e.zoom(0, which=which)
            assert ei.value.code == 1 and "full-f" in str(ei.value) and "which = %d" % which in str(ei.value)
        got = e.zoom(0, which=3)
        assert list(got) == ["markr", "total", "x_edges", "v_edges"] and got["markr"].sum() == e.local_sizes()[1]
        for kw in (dict(x=(0.0, 2 * e.inp.lx)), dict(v=(1.0, 1.0)), dict(v=(0.0, math.inf)), dict(bins=(0, 4)), dict(bins=(4097, 4)),
                   dict(bins=(2048, 513)), dict(ispecies=1), dict(which=0), dict(which=8)):
            with pytest.raises(amd.Pic1dpError) as ei:
                e.zoom(**dict(dict(which=1), **kw))
            assert ei.value.code == 1, kw
        assert e.zoom_stats()[1] == 1
    finally:
        e.close()
    fresh = amd.Pic1dp(amd.make_input(nparticle_max=1000, nx=16))                    # no markers yet
    try:
        with pytest.raises(amd.Pic1dpError) as ei:
            fresh.zoom(0)
        assert "no particles" in str(ei.value)
    finally:
        fresh.close()


# ---------------------------------------------------------------------------
# 6. nothing changes between steps; inside a step the noted push is materialised
# ---------------------------------------------------------------------------
def test_between_steps_nothing_changes(amd, monkeypatch):
    monkeypatch.setenv("PIC1DP_PREDICT", "1")
    monkeypatch.setenv("PIC1DP_PRED_KIND", "2")
    monkeypatch.setenv("PIC1DP_FUSE_SOLVE", "2")
    a, b, c = (G.started(amd, nparticle_max=96, nx=32) for _ in range(3))
    try:
        for e in (a, b, c):
            assert e.predict_kind() == 2
            e.kernel_stats_enable(True)
            e.step(5)
        lx = a.inp.lx
        kwz = dict(x=(0.75 * lx, 0.25 * lx), v=(-4.0, 6.0), bins=(160, 160))
        limbs, got = a.zoom_local_exact(0, **kwz), a.zoom(0, **kwz)
        npass = len(range(0, 160, 40))
        assert a.zoom_stats()[1] == 2 * npass and b.zoom_stats()[1] == 0
        g = G.valid(c)                                # a third context's markers after the same five steps
        ref = Z.reference(g["x"], g["v"], g["p"], g["w"], lx, kwz["x"], kwz["v"], kwz["bins"], 7, *quanta(amd, c.inp))
        Z.assert_same(limbs, ref, "after five steps")
        assert np.any(limbs) and got["pertb"].tobytes() == ref["doubles"][2].tobytes()
        for e in (a, b):
            e.step(5)
        for e in (a, b):
            assert e.kernel_stats(7)[1] == 8                                # all but the last step of each call
            assert e.kernel_stats(3)[1] == 1 and e.kernel_stats(6)[1] == 10    # one first-sub-step pass: the run's first step
        assert a.state_digest().tolist() == b.state_digest().tolist()
        fa, fb = a.get_field(), b.get_field()
        for k in ("electric", "chargeden", "mode_re", "mode_im"):
            assert fa[k].tobytes() == fb[k].tobytes(), k
        assert a.energy_history().tobytes() == b.energy_history().tobytes()
        assert a.get_field_half().tobytes() == b.get_field_half().tobytes()
    finally:
        for e in (a, b, c):
            e.close()


def test_at_every_boundary_of_the_six_calls_lazy_and_eager_engines_agree(amd, monkeypatch):
    kw = dict(nparticle_max=50_001, nx=96)
    monkeypatch.setenv("PIC1DP_PREDICT", "1")
    monkeypatch.setenv("PIC1DP_PRED_KIND", "2")
    a = G.started(amd, **kw)
    monkeypatch.setenv("PIC1DP_PREDICT", "0")
    monkeypatch.delenv("PIC1DP_PRED_KIND")
    monkeypatch.setenv("PIC1DP_LAZY_CALLS", "0")
    b = G.started(amd, **kw)
    monkeypatch.delenv("PIC1DP_LAZY_CALLS")
    try:
        b.set_electric(a.get_field()["electric"])
        lx = a.inp.lx
        kwz = dict(x=(0.6 * lx, 0.1 * lx), v=(2.0, 7.0), bins=(160, 160))
        for e in (a, b):
            e.kernel_stats_enable(True)

        def same(where):
            la, lb = a.zoom_local_exact(0, **kwz), b.zoom_local_exact(0, **kwz)
            assert np.any(la) and np.array_equal(la, lb), where
            return la

        for it in range(2):
            same((it, "step start"))
            for irk in (1, 2):
                for e in (a, b):
                    e.interaction_push_particle(irk)
                if irk == 1 and it == 0:
                    # the lazy context has only noted its push: the call materialises it (a marker kernel runs); the eager one launches none
                    before = [G.marker_launches(e) for e in (a, b)]
                    same((it, irk, "push"))
                    assert G.marker_launches(a) > before[0] and G.marker_launches(b) == before[1]
                    check(amd, b, kwz["x"], kwz["v"], kwz["bins"], masks=(7,), what="eager, inside step %d" % it)
                else:
                    same((it, irk, "push"))
                for e in (a, b):
                    e.interaction_collect_charge()
                same((it, irk, "collect_charge"))
                for e in (a, b):
                    e.field_solve_electric()
                fa, fb = a.get_field(), b.get_field()
                assert np.max(np.abs(fa["electric"] - fb["electric"])) <= 1e-11 * np.max(np.abs(fb["electric"])), (it, irk)
                b.set_electric(fa["electric"])
                same((it, irk, "solve_field"))
        assert a.state_digest().tolist() == b.state_digest().tolist()
    finally:
        a.close()
        b.close()
