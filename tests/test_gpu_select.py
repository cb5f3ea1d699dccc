"""Select and gather markers on the GPU (include/pic1dp_hip.h pic1dp_hip_select, pic1dp_hip_gather) against
tests/select_reference.py: the rule in numpy on the downloaded arrays.  Everything is compared bit for bit -- count, index
and the stored bits of x, v, p, w; there is no tolerance anywhere.  Contexts hold crafted markers (uploaded) whose tail
slots are filled with junk that lies INSIDE the window, so a kernel that reads the tail shows."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import select_reference as R

pytestmark = pytest.mark.gpu

ERR_ARG = 1
CHUNK = 2 * 8192                      # markers of a chunk (pic1dp_amd/csrc/kernels.hpp SELECT_CHUNK_PAIRS; pinned below)
TAIL = 5                              # tail slots of an uploaded context
IN, OUT = 1.0, 5.0                    # velocities inside and outside the window V
V = (0.0, 2.0)


def test_chunk_constant_is_the_librarys(probe):
    assert 2 * probe.host_select_plan(1, 256)["chunk_pairs"] == CHUNK


def uploaded(amd, x, v, p, w, tail=TAIL, **kw):
    """a context holding exactly these markers as its valid ones; the tail slots hold junk inside every window used here"""
    n = len(x)
    kw.setdefault("nx", 16)
    e = amd.Pic1dp(amd.make_input(nparticle_max=n + tail, **kw))
    nalloc, _ = e.local_sizes()
    assert nalloc >= n + tail
    junk = (0.5 * e.inp.lx, IN, -7.0, -9.0)
    arrs = []
    for k, a in enumerate((x, v, p, w)):
        full = np.full(nalloc, junk[k])
        full[:n] = a
        arrs.append(full)
    e.particles_upload(*arrs, np_valid=n)
    return e


def valid(e, s=0):
    g = e.particles_download(s)
    n = e.local_sizes(s)[1]
    return {k: a[:n] for k, a in g.items()}, g


def markers(n, lx, seed=1):
    """n distinct markers with x in [0, lx) and recognisable p, w"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, lx, n), np.full(n, OUT), np.arange(n) + 0.25, -(np.arange(n) + 0.5)


# ---------------------------------------------------------------------------
# 1. sizes x masks
# ---------------------------------------------------------------------------
SIZES = [0, 1, 2, 3, 127, 128, 129, 2047, 2048, 2049, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1]


def masks(n):
    """(name, boolean mask): none, all, alternating, the last marker only, one marker per chunk, a whole chunk empty between
    two full ones"""
    idx = np.arange(n)
    out = [("none", np.zeros(n, bool)), ("all", np.ones(n, bool)), ("alternating", idx % 2 == 1), ("alternating_even", idx % 2 == 0),
           ("last", idx == n - 1)]
    per_chunk = np.zeros(n, bool)
    per_chunk[(idx % CHUNK) == (idx // CHUNK * 4099 + 77) % CHUNK] = True       # another lane, wave and trip in each chunk
    out.append(("one_per_chunk", per_chunk))
    out.append(("middle_chunk_empty", ~((idx >= CHUNK) & (idx < 2 * CHUNK))))
    out.append(("first_of_pair_in_wave_63", (idx % 128) == 126))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_masks(amd, n):
    lx = amd.make_input(nparticle_max=1, nx=16).lx
    x, v, p, w = markers(n, lx, seed=n + 1)
    e = uploaded(amd, x, v, p, w)
    try:
        for name, m in masks(n):
            v = np.where(m, IN, OUT)
            full = [np.concatenate([a, np.full(e.local_sizes()[0] - n, j)]) for a, j in zip((x, v, p, w), (0.5 * lx, IN, -7.0, -9.0))]
            e.particles_upload(*full, np_valid=n)
            ref = R.select(dict(x=x, v=v, p=p, w=w), lx, v_window=V)
            assert ref["count"] == int(m.sum())
            assert e.select_count(0, v=V) == ref["count"], name
            for threads in (0, 1024, 192):               # the library's one-wave workgroups; sixteen waves whose totals go
                e.set_launch(threads, 0)                 # through the LDS; three waves, whose trips do not divide a chunk
                got = e.select(0, v=V)
                R.assert_same(got, ref, what="n %d %s, %d threads" % (n, name, threads))
            e.set_launch(0, 0)
            got = e.select(0, v=V, fraction=0.5, key=n)              # the hash on top, at this size's ranks
            R.assert_same(got, R.select(dict(x=x, v=v, p=p, w=w), lx, v_window=V, thin=2**63, key=n), what="n %d %s thinned" % (n, name))
    finally:
        e.close()


def test_workgroups_that_take_several_chunks(amd):
    """more chunks than workgroups (one workgroup per CU asked for by hand): the grid-stride walk, the loads issued across a
    chunk's end, and the write pass skipping the chunks that hold nothing, at the smallest size that has them"""
    n = 300 * CHUNK + 1
    e = amd.Pic1dp(amd.make_input(nparticle_max=n, nx=64))
    try:
        e.particle_load_device(1)
        e.set_launch(1024, 1)
        g, _ = valid(e)
        lx = e.inp.lx
        for kw in (dict(x=(0.95 * lx, 0.05 * lx), v=(3.0, 4.0)), dict(v=(5.5, np.inf)), dict(fraction=1.0 / 64.0, key=5)):
            ref = R.select(g, lx, x_window=kw.get("x", (-np.inf, np.inf)), v_window=kw.get("v", (-np.inf, np.inf)),
                           thin=R.thin_of(kw.get("fraction", 1.0)), key=kw.get("key", 0))
            assert ref["count"] > 0
            R.assert_same(e.select(0, **kw), ref, what=str(kw))
            R.assert_same(e.select(0, max=1000, **kw), ref, upto=1000, what=str(kw))
        # a window only markers of a few chunks lie in: indices [5 CHUNK + 3, 5 CHUNK + 40) and the last marker
        few = np.zeros(n, bool)
        few[5 * CHUNK + 3:5 * CHUNK + 40] = True
        few[n - 1] = True
        g2 = {k: a.copy() for k, a in g.items()}
        g2["v"] = np.where(few, 100.0, g["v"])
        e.particles_upload(g2["x"], g2["v"], g2["p"], g2["w"])
        R.assert_same(e.select(0, v=(99.0, 101.0)), R.select(g2, lx, v_window=(99.0, 101.0)), what="few chunks")
    finally:
        e.close()


# ---------------------------------------------------------------------------
# 2. crafted markers, every window
# ---------------------------------------------------------------------------
V_LO, V_HI = -1.5, 2.25


@pytest.fixture(scope="module")
def crafted(amd):
    lx = amd.make_input(nparticle_max=1, nx=16).lx
    x, v, p, w = R.edge_markers(lx, V_LO, V_HI)
    e = uploaded(amd, x, v, p, w)
    yield e, dict(x=x, v=v, p=p, w=w)
    e.close()


def test_crafted_markers_and_all_windows(amd, crafted):
    e, g = crafted
    lx = e.inp.lx
    down, _ = valid(e)
    for k in "xvpw":
        assert R.same_bits(down[k], g[k])                    # NaN, -0.0 and 7.3 lx are stored as they came
    for name, xw, vw in R.windows(lx, V_LO, V_HI):
        for fraction, key in ((1.0, 0), (0.25, 3)):
            thin = R.thin_of(fraction)
            ref = R.select(g, lx, x_window=xw, v_window=vw, thin=thin, key=key)
            got = e.select(0, x=xw, v=vw, fraction=fraction, key=key, origin=0)
            R.assert_same(got, ref, what=name)
            count, index = amd.host_select(e.inp, g["x"], g["v"], xw, vw, fraction=fraction, key=key)
            assert count == got["count"] and np.array_equal(index, got["index"]), name
            assert e.select_count(0, x=xw, v=vw, fraction=fraction, key=key, origin=0) == ref["count"]
            print("select %s fraction %g: %d of %d" % (name, fraction, got["count"], g["x"].size))


# ---------------------------------------------------------------------------
# 3. truncation, poisoned buffers, NULL outputs
# ---------------------------------------------------------------------------
def raw_select(e, amd, sel, max_, n_alloc, give=(1, 1, 1, 1, 1)):
    """pic1dp_hip_select into poisoned buffers of n_alloc elements; give[k] = 0 passes NULL for array k (index, x, v, p, w)"""
    index = np.full(n_alloc, -77, dtype=np.int64)
    arrs = [np.full(n_alloc, -77.5) for _ in range(4)]
    bufs = [index] + arrs
    n = C.c_int64(-5)
    rc = e.L.pic1dp_hip_select(e._ctx, 0, C.byref(sel), max_, C.byref(n), *[b.ctypes.data if gv else None for b, gv in zip(bufs, give)])
    return rc, n.value, bufs


def test_truncation_and_null_outputs(amd, crafted):
    e, g = crafted
    lx = e.inp.lx
    xw, vw = (0.0, lx), (V_LO, V_HI)
    ref = R.select(g, lx, x_window=xw, v_window=vw)
    count = ref["count"]
    assert count > 3
    sel = amd.engine.make_select(xw, vw)
    names = ("index", "x", "v", "p", "w")
    for m in (0, 1, count - 1, count, count + 1):
        rc, n, bufs = raw_select(e, amd, sel, m, m + 1)
        k = min(m, count)
        assert rc == 0 and n == count, m
        for name, b in zip(names, bufs):
            assert R.same_bits(b[:k], ref[name][:k]), (m, name)
            assert np.all(b[k:] == (-77 if name == "index" else -77.5)), (m, name)    # the poison behind them is intact
        R.assert_same(e.select(0, x=xw, v=vw, max=m), ref, upto=m)
    for left_out in range(5):
        give = [1] * 5
        give[left_out] = 0
        rc, n, bufs = raw_select(e, amd, sel, count, count + 1, give)
        assert rc == 0 and n == count
        for j, (name, b) in enumerate(zip(names, bufs)):
            if give[j]:
                assert R.same_bits(b[:count], ref[name]) and np.all(b[count:] == (-77 if name == "index" else -77.5)), (left_out, name)
            else:
                assert np.all(b == (-77 if name == "index" else -77.5)), (left_out, name)
    rc, n, bufs = raw_select(e, amd, sel, count, count + 1, (0, 0, 0, 0, 0))
    assert rc == 0 and n == count


# ---------------------------------------------------------------------------
# 4. launch shape
# ---------------------------------------------------------------------------
def test_launch_shape_does_not_show(amd):
    n = 3 * CHUNK + 1
    lx = amd.make_input(nparticle_max=1, nx=16).lx
    rng = np.random.default_rng(5)
    x, v, p, w = rng.uniform(-lx, 2 * lx, n), rng.normal(0.0, 2.0, n), rng.normal(size=n), rng.normal(size=n)
    e = uploaded(amd, x, v, p, w)
    try:
        kw = dict(x=(0.7 * lx, 0.3 * lx), v=(-1.0, 3.0), fraction=0.5, key=2)
        ref = R.select(dict(x=x, v=v, p=p, w=w), lx, x_window=kw["x"], v_window=kw["v"], thin=2**63, key=2)
        assert ref["count"] > 1000
        first = None
        for threads, bpc in itertools.product((0, 64, 256, 1024), (0, 1, 4)):
            e.set_launch(threads, bpc)
            got = e.select(0, **kw)
            R.assert_same(got, ref, what="%d x %d" % (threads, bpc))
            blob = b"".join(got[k].tobytes() for k in ("index", "x", "v", "p", "w"))
            first = first or blob
            assert blob == first
    finally:
        e.close()


# ---------------------------------------------------------------------------
# 5. gather
# ---------------------------------------------------------------------------
def test_gather(amd, crafted):
    e, g = crafted
    nalloc, np_ = e.local_sizes()
    assert nalloc >= np_ + TAIL
    _, full = valid(e)
    rng = np.random.default_rng(3)
    e.kernel_stats_enable(True)
    for n in (0, 1, 63, 64, 65, 4097):
        cases = {"ascending": np.arange(n) % nalloc, "reversed": (nalloc - 1 - np.arange(n)) % nalloc,
                 "random_with_duplicates": rng.integers(0, nalloc, n), "all_the_same": np.full(n, np_ - 1),
                 "tail_slots": np_ + np.arange(n) % (nalloc - np_)}
        for name, idx in cases.items():
            before = e.kernel_stats(22)[1]
            got = e.gather(0, idx)
            assert e.kernel_stats(22)[1] == before + (1 if n else 0), (n, name)
            for k in "xvpw":
                assert got[k].shape == (n,) and R.same_bits(got[k], full[k][idx]), (n, name, k)
    idx = np.array([3, 1, 2], dtype=np.int64)      # NULL outputs: the others are still served
    vv = np.full(3, -77.5)
    assert e.L.pic1dp_hip_gather(e._ctx, 0, idx.ctypes.data, 3, None, vv.ctypes.data, None, None) == 0
    assert R.same_bits(vv, full["v"][idx])
    for bad in (-1, nalloc):
        before = e.kernel_stats(22)[1]
        with pytest.raises(amd.Pic1dpError) as ei:
            e.gather(0, [0, 5, bad, -3])
        assert ei.value.code == ERR_ARG and "index[2] = %d" % bad in str(ei.value)
        assert e.kernel_stats(22)[1] == before                # nothing launched
    with pytest.raises(amd.Pic1dpError):
        e.gather(1, [0])                                       # unknown species
    e.kernel_stats_enable(False)


# ---------------------------------------------------------------------------
# 6. in a run
# ---------------------------------------------------------------------------
RUN_N = 2**18 + 1


def run_window(lx):
    return dict(x=(0.9 * lx, 0.1 * lx), v=(3.0, 4.0), fraction=1.0 / 8.0, key=4)


def check_against_download(e, what, select_first=True):
    kw = run_window(e.inp.lx)
    got = e.select(0, **kw) if select_first else None
    g, _ = valid(e)
    if got is None:
        got = e.select(0, **kw)
    ref = R.select(g, e.inp.lx, x_window=kw["x"], v_window=kw["v"], thin=R.thin_of(kw["fraction"]), key=kw["key"],
                   origin=0)
    assert ref["count"] > 20, what
    R.assert_same(got, ref, what=what)
    print("run %s: %d selected" % (what, got["count"]))
    return got


@pytest.mark.parametrize("sites", ["lazy", "eager"])
def test_in_a_run(amd, monkeypatch, sites):
    monkeypatch.setenv("PIC1DP_LAZY_CALLS", "1" if sites == "lazy" else "0")
    e = amd.Pic1dp(amd.make_input(nparticle_max=RUN_N, nx=64))
    try:
        e.particle_load_device(1)
        e.interaction_collect_charge()
        e.field_solve_electric()
        check_against_download(e, "start")
        for step in range(3):
            # the reference's call sites, with a look at the markers while push(1) is only noted
            e.interaction_push_particle(1)
            first = check_against_download(e, "%s step %d, push(1) noted" % (sites, step))
            e.interaction_collect_charge()
            e.field_solve_electric()
            e.interaction_push_particle(2)
            e.interaction_collect_charge()
            e.field_solve_electric()
            second = check_against_download(e, "%s step %d, between steps" % (sites, step), select_first=step % 2 == 0)
            assert first["count"] > 0 and second["count"] > 0
        # the tracer use: a thinned sample of everything, followed over steps
        tracers = e.select(0, fraction=1.0 / 512.0, key=8)
        assert 300 < tracers["count"] < 800
        e.step(2)
        g, _ = valid(e)
        got = e.gather(0, tracers["index"])
        for k in "xvpw":
            assert R.same_bits(got[k], g[k][tracers["index"]]), k
        assert R.same_bits(got["p"], tracers["p"]) and not R.same_bits(got["x"], tracers["x"])
        again = e.select(0, fraction=1.0 / 512.0, key=8)
        assert np.array_equal(again["index"], tracers["index"])          # the same markers at every time
    finally:
        e.close()


# ---------------------------------------------------------------------------
# 7. nothing changes between steps
# ---------------------------------------------------------------------------
def test_nothing_changes_between_steps(amd, monkeypatch):
    """around a select_count, selects and a gather between two steps: the step kernels' launch counters, the one-pass
    prediction, the fused solve and the state digest are what they were, and the run is the run of a twin that never asked,
    bit for bit (96 markers, nx 32, as tests/test_gpu_checkpoint.py: at most one wave of markers, so the step's FP64 sums
    have one order and two contexts can be compared bit for bit at all)"""
    monkeypatch.setenv("PIC1DP_PREDICT", "1")
    monkeypatch.setenv("PIC1DP_PRED_KIND", "2")
    monkeypatch.setenv("PIC1DP_FUSE_SOLVE", "2")

    def fresh():
        e = amd.Pic1dp(amd.make_input(nparticle_max=96, nx=32))
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()
        e.kernel_stats_enable(True)
        e.step(5)
        return e

    e, twin = fresh(), fresh()
    try:
        e.sync()
        counters = lambda c: [c.kernel_stats(k)[1] for k in (0, 1, 2, 3, 4, 6, 7)]
        before = (counters(e), e.predict_kind(), e.state_digest().tobytes())
        assert before[1] == 2
        s21, s22 = e.kernel_stats(21)[1], e.kernel_stats(22)[1]
        kw = dict(x=(0.75 * e.inp.lx, 0.5 * e.inp.lx), fraction=0.5, key=4)
        n = e.select_count(0, **kw)
        assert e.kernel_stats(21)[1] == s21 + 1
        got = e.select(0, max=n, **kw)
        g, _ = valid(e)
        R.assert_same(got, R.select(g, e.inp.lx, x_window=kw["x"], thin=2**63, key=4))
        assert got["count"] == n > 10 and e.kernel_stats(21)[1] == s21 + 3
        assert e.select(0, max=0, **kw)["count"] == n and e.kernel_stats(21)[1] == s21 + 4      # max = 0 equals select_count
        assert e.select(0, v=(50.0, 60.0))["count"] == 0 and e.kernel_stats(21)[1] == s21 + 6   # (max=None counts first) nothing to write
        e.gather(0, got["index"])
        assert e.kernel_stats(22)[1] == s22 + 1
        assert e.kernel_stats(21)[0] > 0.0 and e.kernel_stats(22)[0] > 0.0                      # device milliseconds while stats are enabled
        assert (counters(e), e.predict_kind(), e.state_digest().tobytes()) == before
        e.check_state(True)
        for c in (e, twin):
            c.step(5)
        assert e.kernel_stats(3)[1] == 1 and e.kernel_stats(6)[1] == 10 and e.kernel_stats(7)[1] == 8   # still one pass, one launch per step
        assert counters(e) == counters(twin)
        assert e.field_energy() == twin.field_energy()
        assert e.energy_history().tobytes() == twin.energy_history().tobytes()
        assert e.state_digest().tobytes() == twin.state_digest().tobytes()
        fa, fb = e.get_field(), twin.get_field()
        for k in ("electric", "chargeden", "mode_re", "mode_im"):
            assert fa[k].tobytes() == fb[k].tobytes(), k
    finally:
        e.close()
        twin.close()


# ---------------------------------------------------------------------------
# 8. species and layout
# ---------------------------------------------------------------------------
def test_two_species_and_four_blocks_in_one_context(amd):
    kw = dict(nparticle_max=40_007, nx=64, nspecies=2, species_nparticle_init=[40_001, 23_456], species_charge=[-1.0, 1.0],
              species_mass=[1.0, 4.0], species_temperature=[1.0, 1.0], species_temperature2=[1.0, 1.0],
              species_density=[0.9, 0.9], species_v0=[5.0, 5.0])
    e = amd.Pic1dp(amd.make_input(**kw), npe=4)
    try:
        e.particle_load_device(1)
        lx = e.inp.lx
        for s in (0, 1):
            g, full = valid(e, s)
            assert g["x"].size == kw["species_nparticle_init"][s]
            ref = R.select(g, lx, x_window=(0.5 * lx, 0.25 * lx), v_window=(-2.0, 6.0), thin=2**62, key=1)
            assert ref["count"] > 100
            R.assert_same(e.select(s, x=(0.5 * lx, 0.25 * lx), v=(-2.0, 6.0), fraction=0.25, key=1), ref, what="species %d" % s)
            idx = np.array([0, g["x"].size - 1, g["x"].size, full["x"].size - 1, 17, 17])
            got = e.gather(s, idx)
            for k in "xvpw":
                assert R.same_bits(got[k], full[k][idx]), (s, k)
        with pytest.raises(amd.Pic1dpError):
            e.gather(1, [e.local_sizes(1)[0]])
    finally:
        e.close()


def test_tail_slots_live_in_set_0_while_the_other_set_is_current(amd):
    """after an odd number of substep calls the valid markers are in the second marker set and the tail slots still in set 0
    (pic1dp_hip_particles_download): gather takes each index from where download takes it, select reads the current set"""
    e = amd.Pic1dp(amd.make_input(nparticle_max=5000, nx=32, species_nparticle_init=[4097]))
    try:
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()
        nalloc, np_ = e.local_sizes()
        assert np_ == 4097 < nalloc
        before, full0 = valid(e)
        e.step(3)
        e.substep(1)
        g, full = valid(e)
        assert not R.same_bits(g["x"], before["x"])
        assert np.any(full["x"][np_:] != 0.0)                 # the host load left markers in the tail slots: something to get wrong
        idx = np.concatenate([np.arange(np_ - 40, nalloc), np.arange(nalloc - 1, np_ - 3, -1), [0, np_, np_ - 1, np_]])
        got = e.gather(0, idx)
        for k in "xvpw":
            assert R.same_bits(got[k], full[k][idx]), k
        ref = R.select(g, e.inp.lx, v_window=(-1.0, 2.0), thin=2**63, key=2)
        R.assert_same(e.select(0, v=(-1.0, 2.0), fraction=0.5, key=2), ref)
        e.substep(2)
        g, full = valid(e)
        got = e.gather(0, idx)
        for k in "xvpw":
            assert R.same_bits(got[k], full[k][idx]), k
    finally:
        e.close()


def test_full_f_context(amd):
    e = amd.Pic1dp(amd.make_input(nparticle_max=20_001, nx=64, deltaf=0))
    try:
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()
        e.step(1)
        g, full = valid(e)
        ref = R.select(g, e.inp.lx, v_window=(1.0, np.inf), thin=2**63, key=0)
        R.assert_same(e.select(0, v=(1.0, np.inf), fraction=0.5), ref, what="full f")       # w: whatever download gives
        idx = np.arange(0, e.local_sizes()[0], 97)
        got = e.gather(0, idx)
        for k in "xvpw":
            assert R.same_bits(got[k], full[k][idx]), k
    finally:
        e.close()


def test_default_origin_makes_a_sample_independent_of_the_split_over_ranks(amd):
    kw = dict(nparticle_max=3 * 4096 + 5, nx=64)
    one = amd.Pic1dp(amd.make_input(**kw))
    two = [amd.Pic1dp(amd.make_input(**kw), rank=r, nranks=2) for r in range(2)]
    try:
        for e in [one] + two:
            e.particle_load_device(1)
        lx = one.inp.lx
        sel = dict(x=(0.8 * lx, 0.4 * lx), v=(-3.0, 3.0), fraction=0.125, key=6)
        whole = one.select(0, **sel)
        assert whole["count"] > 100
        g0 = [amd.load_origin(one.inp, 0, rank=r, nranks=2) for r in range(2)]
        assert g0[0] == 0 < g0[1]
        parts = [e.select(0, **sel) for e in two]
        for r, (e, part) in enumerate(zip(two, parts)):
            R.assert_same(e.select(0, origin=g0[r], **sel), part)                # the default origin is load_origin
        assert parts[0]["count"] + parts[1]["count"] == whole["count"]
        assert np.array_equal(np.concatenate([parts[0]["index"], parts[1]["index"] + g0[1]]), whole["index"])
        for k in "xvpw":
            assert R.same_bits(np.concatenate([parts[0][k], parts[1][k]]), whole[k]), k
        other = two[1].select(0, origin=0, **sel)                                 # without it the second half keeps other markers
        assert not np.array_equal(other["index"], parts[1]["index"])
    finally:
        for e in [one] + two:
            e.close()


# ---------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------
def test_errors_leave_the_context_untouched(amd, crafted):
    e, g = crafted
    digest = e.state_digest().tobytes()
    s21 = e.kernel_stats(21)[1]
    good = amd.engine.make_select()
    n = C.c_int64(-5)
    buf = np.full(8, -77.5)
    L = e.L

    def refused(rc, word):
        assert rc == ERR_ARG and word in L.pic1dp_hip_last_error().decode(), (rc, word, L.pic1dp_hip_last_error())
        assert n.value == -5 and np.all(buf == -77.5)

    refused(L.pic1dp_hip_select(e._ctx, 1, C.byref(good), 8, C.byref(n), None, buf.ctypes.data, None, None, None), "species")
    refused(L.pic1dp_hip_select(e._ctx, -1, C.byref(good), 8, C.byref(n), None, buf.ctypes.data, None, None, None), "species")
    refused(L.pic1dp_hip_select(e._ctx, 0, C.byref(good), -1, C.byref(n), None, buf.ctypes.data, None, None, None), "negative")
    refused(L.pic1dp_hip_select(e._ctx, 0, None, 8, C.byref(n), None, buf.ctypes.data, None, None, None), "null")
    assert L.pic1dp_hip_select(e._ctx, 0, C.byref(good), 8, None, None, buf.ctypes.data, None, None, None) == ERR_ARG
    for field in ("x_lo", "x_hi", "v_lo", "v_hi"):
        bad = amd.engine.make_select()
        setattr(bad, field, math.nan)
        refused(L.pic1dp_hip_select(e._ctx, 0, C.byref(bad), 8, C.byref(n), None, buf.ctypes.data, None, None, None), "NaN")
        refused(L.pic1dp_hip_select_count(e._ctx, 0, C.byref(bad), C.byref(n)), "NaN")
    with pytest.raises(amd.Pic1dpError):
        e.select(0, fraction=0.0)
    assert L.pic1dp_hip_gather(e._ctx, 0, None, 3, buf.ctypes.data, None, None, None) == ERR_ARG
    assert L.pic1dp_hip_gather(e._ctx, 0, None, -1, buf.ctypes.data, None, None, None) == ERR_ARG
    assert L.pic1dp_hip_gather(e._ctx, 0, None, 0, buf.ctypes.data, None, None, None) == 0      # n = 0: a no-op
    assert np.all(buf == -77.5)
    assert e.kernel_stats(21)[1] == s21 and e.state_digest().tobytes() == digest
    e.check_state(True)
    ref = R.select(g, e.inp.lx)
    R.assert_same(e.select(0, origin=0), ref)                                                   # and it still serves


def test_no_markers_loaded_is_a_state_error(amd):
    e = amd.Pic1dp(amd.make_input(nparticle_max=100, nx=16))
    try:
        with pytest.raises(amd.Pic1dpError) as ei:
            e.select(0)
        assert ei.value.code == 4
        with pytest.raises(amd.Pic1dpError) as ei:
            e.gather(0, [1])
        assert ei.value.code == 4
    finally:
        e.close()
