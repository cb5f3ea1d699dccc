"""The exact diagnostics sum (kind 1 of include/pic1dp_hip.h set_diag_sum) on the GPU: the pass against
the numpy restatement (tests/diag_exact.py) bit for bit, independence of marker order, flush windows, rank split, API
path; the bytes of pic1dp.out; kind 0 untouched; the loud overflow; the state rules."""
import math

import numpy as np
import pytest

import diag_exact as dx
import diag_reference as dr

pytestmark = pytest.mark.gpu

N = 4099                  # odd, and more than one trip of a workgroup's 2 x 1024 markers
PLANES = dr.PLANES
TWO = dict(nspecies=2, species_charge=[-1.0, 1.0], species_mass=[1.0, 4.0], species_temperature=[1.0, 0.5],
           species_temperature2=[1.0, 0.5], species_density=[1.0, 1.0], species_v0=[0.0, 0.0], iptcldist=0,
           species_nparticle_init=[N, 2053])
FULLF = dict(deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0])
CASES = {"deltaf": dict(), "fullf": FULLF, "two": TWO}


def make(amd, n=N, nxo=64, nvo=64, **kw):
    inp = amd.make_input(**dict(dict(nparticle_max=n, nx=64, nx_opd=nxo, nv_opd=nvo), **kw))
    return inp, amd.Pic1dp(inp, device=0)


def crafted(amd, inp, eng, s):
    """the loader's markers of species s (within B_s by construction) with, in the first slots: the edge markers of
    diag_reference (x = lx, the top v row, one ulp either side of +-v_max), |v| in (v_max, 30 v_max), and weights whose
    terms lie on rounding ties.  Returns x, v, p, w over all slots and the number of valid markers"""
    na, npv = eng.local_sizes(s)
    d = eng.particles_download(s)
    x, v, p, w = d["x"].copy(), d["v"].copy(), d["p"].copy(), d["w"].copy()
    e = amd.diag_quanta(inp, s)
    bound = 2.0 ** (amd.charge_quantum(inp, s) + 52)
    ex, ev, ep, ew = dr.edge_markers(inp.lx, inp.v_max, inp.nx_opd, inp.nv_opd, seed=7 + s)
    m = min(len(ex), npv // 4)
    x[:m], v[:m], p[:m], w[:m] = ex[:m], ev[:m], ep[:m] * bound / 4.0, ew[:m] * bound / 4.0
    far = np.array([1.5, -7.0, 29.9, -1.0 - 2.0 ** -52, 1.0 + 2.0 ** -52, 12.25]) * inp.v_max
    v[m:m + far.size] = far
    m += far.size
    # x = 0 and a top-row velocity: the weights are 1, 0, 0, 0, so p and w ARE the terms -- half-way between two quanta
    tops = dr.top_velocities(inp.v_max, inp.nv_opd)[:4]
    for j, vt in enumerate(tops):
        x[m], v[m] = 0.0, vt
        p[m] = (2.0 ** 20 + j + 0.5) * 2.0 ** e[1]
        w[m] = -(2.0 ** 21 + j + 0.5) * 2.0 ** e[2]
        m += 1
    assert m <= npv
    # the tail slots count in the kinetic sums only
    nt = na - npv
    x[npv:], v[npv:] = 0.5 * inp.lx, np.linspace(-2.0, 2.0, nt) * inp.v_max
    p[npv:], w[npv:] = bound / 8.0, np.linspace(-1.0, 1.0, nt) * bound / 16.0
    return x, v, p, w, npv


def restatement(amd, inp, s, markers):
    x, v, p, w, npv = markers
    ref = dx.exact(x, v, p, w, npv, inp.lx, inp.v_max, inp.nx_opd, inp.nv_opd, inp.deltaf, amd.diag_quanta(inp, s))
    assert ref["rejected"] == [0] * 6
    return ref


def diagnostics(eng, ns):
    """everything the pass serves, by every call that serves it"""
    out = dict(raw=[eng.ptcldist(s, finish=False) for s in range(ns)], sums=[eng.energy_sums(s) for s in range(ns)],
               fin=[eng.ptcldist(s, finish=True) for s in range(ns)], scal=eng.output_scalars())
    out["all_scal"], _, out["all_dist"] = eng.output_all()
    return out


def same_diagnostics(a, b, ns):
    ok = np.array_equal(a["scal"], b["scal"]) and np.array_equal(a["all_scal"], b["all_scal"])
    for s in range(ns):
        ok = ok and np.array_equal(a["sums"][s], b["sums"][s])
        for k in PLANES:
            ok = ok and all(np.array_equal(a[key][s][k], b[key][s][k]) for key in ("raw", "fin", "all_dist"))
    return ok


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(64, 64), (1, 2), (192, 192)], ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("case", list(CASES))
def test_equals_the_definition_bit_for_bit(amd, case, grid):
    """(1 x 2: degenerate corners; 192 x 192: beyond a workgroup's LDS copy, limbs straight into the global rows)"""
    inp, eng = make(amd, nxo=grid[0], nvo=grid[1], **CASES[case])
    ns = inp.nspecies
    eng.particle_load()
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    marks = [crafted(amd, inp, eng, s) for s in range(ns)]
    for s in range(ns):
        x, v, p, w, npv = marks[s]
        eng.particles_upload(x, v, p, w, ispecies=s, np_valid=npv)
    eng.set_diag_sum(1)
    refs = [restatement(amd, inp, s, marks[s]) for s in range(ns)]
    got = diagnostics(eng, ns)
    for s in range(ns):
        assert np.array_equal(got["sums"][s], refs[s]["sums"]), (s, got["sums"][s], refs[s]["sums"])
        for k in PLANES:
            want = refs[s]["raw"][k]
            assert np.array_equal(got["raw"][s][k], want), (s, k, np.flatnonzero(got["raw"][s][k] != want)[:4])
        fin = eng.ptcldist_finish(refs[s]["raw"], s)
        for k in PLANES:
            assert np.array_equal(got["fin"][s][k], fin[k]) and np.array_equal(got["all_dist"][s][k], fin[k]), (s, k)
    scal = eng.output_scalars_from(np.concatenate([r["sums"] for r in refs]))
    assert np.array_equal(got["scal"], scal) and np.array_equal(got["all_scal"], scal)
    assert eng.kernel_stats(15)[1] == 0
    eng.check_state(True)


@pytest.mark.parametrize("n", [N, (1 << 18) + 3], ids=["4099", "2^18+3"])
def test_order_of_the_markers_does_not_matter(amd, n):
    """the same markers in a seeded random permutation and in reverse: all six planes and the three sums identical.
    2^18 + 3 markers: workgroups of more than 32 trips, whose LDS copy is flushed inside the loop"""
    inp, eng = make(amd, n=n, **TWO | dict(species_nparticle_init=[n, n // 2 + 1]))
    eng.particle_load()
    marks = [crafted(amd, inp, eng, s) for s in range(2)]
    eng.set_diag_sum(1)
    runs = []
    for order in ("as loaded", "permuted", "reversed"):
        for s in range(2):
            x, v, p, w, npv = marks[s]
            idx = np.arange(x.size)
            if order == "permuted":
                idx[:npv] = np.random.default_rng(17 + s).permutation(npv)
            elif order == "reversed":
                idx[:npv] = idx[:npv][::-1]
            eng.particles_upload(x[idx], v[idx], p[idx], w[idx], ispecies=s, np_valid=npv)
        runs.append(dict(raw=[eng.ptcldist(s, finish=False) for s in range(2)], sums=[eng.energy_sums(s) for s in range(2)]))
    for r in runs[1:]:
        for s in range(2):
            assert np.array_equal(r["sums"][s], runs[0]["sums"][s])
            for k in PLANES:
                assert np.array_equal(r["raw"][s][k], runs[0]["raw"][s][k]), (s, k)
    assert np.count_nonzero(runs[0]["raw"][0]["pertb_xv"]) > 100 and eng.kernel_stats(15)[1] == 0


N_WINDOW = (1 << 18) + 3


def normalised(limbs, nxv):
    """a context's limbs as the host normalises them: hi += lo >> 32, lo &= 2^32 - 1.  (What a context hands out is the sum
    of its workgroups' flushes, limb by limb: how a total splits into hi and lo depends on where the windows fall)"""
    out = np.array(limbs, dtype=np.int64)
    for pairs in (out[:6 * nxv].reshape(3, 2, nxv), out[6 * nxv:6 * nxv + 6].reshape(3, 2, 1)):
        pairs[:, 0] += pairs[:, 1] >> 32
        pairs[:, 1] &= 0xffffffff
    return out


@pytest.fixture(scope="module")
def window_cases(amd):
    """N_WINDOW crafted markers on the 64 x 64 grid, delta f and full f: the markers, the definition's limbs and the limbs
    of a context at the default setting, once"""
    out = {}
    for case in ("deltaf", "fullf"):
        inp, eng = make(amd, n=N_WINDOW, **CASES[case])
        eng.particle_load()
        marks = crafted(amd, inp, eng, 0)
        eng.particles_upload(*marks[:4], np_valid=marks[4])
        eng.set_diag_sum(1)
        want = dx.limbs_of(restatement(amd, inp, 0, marks)["ints"], 64 * 64)
        assert np.array_equal(normalised(want, 64 * 64), want)
        out[case] = (marks, want, normalised(eng.diag_local_exact(0), 64 * 64))
        eng.close()
    return out


@pytest.mark.parametrize("case", ["deltaf", "fullf"])
@pytest.mark.parametrize("drawn", ["0", "16"])
def test_rows_all_dealt_and_all_drawn_then_capped(amd, monkeypatch, tuning, window_cases, drawn, case):
    """tuning knob PIC1DP_DYN_TAIL at its two ends, the branches the shared sweep and window_rows (device_sweep.hpp) own: every
    row of a workgroup dealt, and every row drawn, of which the cap deals all but 31 again.  The normalised limbs are those
    of the default setting and of the definition, bit for bit"""
    marks, want, base = window_cases[case]
    monkeypatch.setenv("PIC1DP_DYN_TAIL", drawn)
    inp, eng = make(amd, n=N_WINDOW, **CASES[case])
    eng.particle_load()
    eng.particles_upload(*marks[:4], np_valid=marks[4])
    eng.set_diag_sum(1)
    got = normalised(eng.diag_local_exact(0), 64 * 64)
    assert np.array_equal(got, base), np.flatnonzero(got != base)[:5]
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    assert np.any(got[:6 * 64 * 64:7]) and eng.kernel_stats(15)[1] == 0


# ---------------------------------------------------------------------------------------------------------------------
RANK_KW = dict(nparticle_max=40_001, nx=64)


def started(amd, **kw):
    eng = amd.Pic1dp(amd.make_input(**RANK_KW), device=0, **kw)
    eng.particle_load()
    eng.set_charge_sum(1)
    eng.set_diag_sum(1)
    return eng


def host_collect(engs):
    tot = sum(e.charge_local_exact() for e in engs)
    for e in engs:
        e.charge_reduced_exact(tot)
        e.field_solve_electric()


class HostReduced:
    """the record of a run split over contexts whose diagnostics limbs the host sums: the three calls OutputWriter uses"""

    def __init__(self, engs):
        self.engs = engs
        self.ns = engs[0].inp.nspecies
        conv = [engs[0].diag_convert_exact(sum(e.diag_local_exact(s) for e in engs), s) for s in range(self.ns)]
        self.sums = np.concatenate([c[0] for c in conv])
        self.raw = [c[1] for c in conv]

    def output_scalars(self):
        return self.engs[0].output_scalars_from(self.sums)

    def get_field(self):
        return self.engs[0].get_field()

    def ptcldist(self, s, finish=True):
        return self.engs[0].ptcldist_finish(self.raw[s], s) if finish else self.raw[s]


def test_rank_split(amd):
    one = started(amd, npe=2)
    one.interaction_collect_charge()
    one.field_solve_electric()
    base = diagnostics(one, 1)
    base_field = one.get_field()
    one.close()       # (at most two contexts at a time)
    engs = [started(amd, rank=r, nranks=2) for r in range(2)]
    host_collect(engs)
    h = HostReduced(engs)
    assert np.array_equal(h.output_scalars(), base["scal"])
    assert np.array_equal(h.sums, base["sums"][0])
    for k in PLANES:
        assert np.array_equal(h.raw[0][k], base["raw"][0][k]), k
        assert np.array_equal(h.ptcldist(0)[k], base["fin"][0][k]) and np.array_equal(h.ptcldist(0)[k], base["all_dist"][0][k]), k
    assert np.array_equal(h.get_field()["electric"], base_field["electric"])
    # a rank's own limbs are its own: finish = 1 without a communicator is refused, as in kind 0
    with pytest.raises(amd.Pic1dpError):
        engs[0].ptcldist(0, finish=True)
    for e in engs:
        e.close()
    # a one-rank RCCL communicator (the limbs through ncclInt64) against none
    a = amd.Pic1dp(amd.make_input(**RANK_KW), device=0)
    b = amd.Pic1dp(amd.make_input(**RANK_KW), device=0)
    b.comm_available()
    b.comm_init(b.comm_unique_id())
    for e in (a, b):
        e.particle_load()
        e.set_charge_sum(1)
        e.set_diag_sum(1)
        e.interaction_collect_charge()
        e.field_solve_electric()
        e.step(3)
    assert same_diagnostics(diagnostics(a, 1), diagnostics(b, 1), 1)


def test_the_file_has_the_same_bytes_on_every_path(amd, tmp_path):
    """charge sum 1 and diagnostics sum 1, ten steps, a record at the start and one at the end, through
    pic1dp_amd/output.py: step(), the lazy call sites, and two contexts whose limbs the host sums"""
    from pic1dp_amd.output import OutputWriter
    steps = 10
    files = []

    def calls(engs, collect):
        for _ in range(steps):
            for irk in (1, 2):
                for e in engs:
                    e.interaction_push_particle(irk)
                collect()
            for e in engs:
                e.set_time(e.itime + 1, e.time + e.inp.dt)

    for path in ("step", "calls", "split"):
        if path == "split":
            engs = [started(amd, rank=r, nranks=2) for r in range(2)]
            collect = lambda: host_collect(engs)                         # noqa: E731
            record = lambda: HostReduced(engs)                           # noqa: E731
        else:
            engs = [started(amd, npe=2)]
            collect = lambda: (engs[0].interaction_collect_charge(), engs[0].field_solve_electric())   # noqa: E731
            record = lambda: engs[0]                                     # noqa: E731
        name = str(tmp_path / (path + ".out"))
        with OutputWriter(name, engs[0].inp) as out:
            collect()
            out.write_record(record())
            if path == "step":
                engs[0].step(steps)
            else:
                calls(engs, collect)
            out.write_record(record())
        for e in engs:
            e.close()
        files.append(open(name, "rb").read())
    assert len(files[0]) > 2 * 8 * 3 * 64 * 64
    assert files[0] == files[1], "step() against the lazy call sites"
    assert files[0] == files[2], "one context against two whose limbs the host sums"


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(64, 64), (192, 192)], ids=lambda g: "%dx%d" % g)
def test_against_kind_0_and_back(amd, grid):
    """both kinds within their bounds of the exact reference.  Switching back restores kind 0: on the LDS path its
    kernel choice (kernel_stats 12) and with it the fixed-point pass's bits; on the LDS-less path its double sums, within
    their bound on the loader's markers and bit for bit where every bin holds one marker (one order of additions)"""
    inp, eng = make(amd, nxo=grid[0], nvo=grid[1])
    lds = 8 * (3 * grid[0] * grid[1] + 3 * grid[1]) <= 150 * 1024
    eng.particle_load()
    d = eng.particles_download()
    ref = dr.reference(d["x"], d["v"], d["p"], d["w"], inp.lx, inp.v_max, grid[0], grid[1], 1)
    first = eng.ptcldist(0, finish=False)              # kind 0, double sums (no bounds known yet)
    eng.interaction_collect_charge()                   # (bumps the marker state; the markers are in [0, lx): unchanged)
    k0 = eng.ptcldist(0, finish=False)                 # kind 0 again: fixed point on the LDS path
    fx0 = eng.kernel_stats(12)[1]
    assert fx0 == (1 if lds else 0)
    eng.set_diag_sum(1)
    k1 = eng.ptcldist(0, finish=False)
    assert eng.kernel_stats(12)[1] == fx0
    e = amd.diag_quanta(inp, 0)
    q0, blocks = dr.dist_quanta(N, 256, 1, 2.0 * np.max(np.abs(d["p"])), 16.0 * np.max(np.abs(d["w"])))
    for j, k in enumerate(PLANES):
        plane = ref[k.replace("_v", "_vrow") if k.endswith("_v") else k]
        assert np.all(dr.error(k1[k], plane) <= dr.fixed_bound(plane, 2.0 ** e[j % 3], 1)), k
        assert np.all(dr.on_grid(k1[k], 2.0 ** e[j % 3])), k
        if lds:
            assert np.all(dr.error(k0[k], plane) <= dr.fixed_bound(plane, q0[j % 3], blocks)), k
        else:
            assert np.all(dr.error(k0[k], ref[k]) <= dr.double_bound(ref[k], 2 * 256)), k
    eng.set_diag_sum(0)
    back = eng.ptcldist(0, finish=False)
    assert eng.kernel_stats(12)[1] == fx0 + (1 if lds else 0)      # the same kernel choice as before the switch
    for k in PLANES:
        if lds:
            assert np.array_equal(back[k], k0[k]), k                  # (fixed-point sums: order-free, the same bits)
        else:
            assert np.all(dr.error(back[k], ref[k]) <= dr.double_bound(ref[k], 2 * 256)), k
    if not lds:
        # one marker per bin at most: the double sums have one order, kind 0 before and after the switch agree bit for bit
        x, v, p, w = dr.edge_markers(inp.lx, inp.v_max, grid[0], grid[1])
        g = dr.batches(x, v, inp.lx, inp.v_max, grid[0], grid[1])[0]
        na = eng.local_sizes()[0]
        X, V = np.full(na, 0.5 * inp.lx), np.full(na, inp.v_max)
        P, W = np.full(na, 0.75), np.full(na, -0.5)
        X[:len(g)], V[:len(g)], P[:len(g)], W[:len(g)] = x[g], v[g], p[g] * 1e-3, w[g] * 1e-3
        eng.particles_upload(X, V, P, W)
        before = eng.ptcldist(0, finish=False)
        eng.set_diag_sum(1)
        eng.ptcldist(0, finish=False)
        eng.set_diag_sum(0)
        after = eng.ptcldist(0, finish=False)
        for k in PLANES:
            assert np.array_equal(before[k], after[k]), k
    assert np.max(np.abs(first["markr_xv"] - k1["markr_xv"])) < 1e-9


def test_overflow_is_loud_and_recoverable(amd):
    """nv_opd = 65: v = 0 lies on a row, and x = 0 on a column -- the marker's weights are 1, 0, 0, 0, so exactly one
    term (1 * w, plane pertb) is beyond the limit; its kinetic terms are zero"""
    inp, eng = make(amd, nvo=65)
    eng.particle_load()
    d = eng.particles_download()
    bound = 2.0 ** (amd.charge_quantum(inp, 0) + 52)
    x, v, p, w = d["x"].copy(), d["v"].copy(), d["p"].copy(), d["w"].copy()
    x[17], v[17], w[17] = 0.0, 0.0, 2.0 ** 12 * bound
    eng.particles_upload(x, v, p, w)
    eng.set_diag_sum(1)
    for call in (lambda: eng.ptcldist(0, finish=False), eng.output_all, lambda: eng.energy_sums(0)):
        with pytest.raises(amd.Pic1dpError) as ex:
            call()
        assert ex.value.code == 1 and "species 0" in str(ex.value) and "pertb" in str(ex.value)
    assert eng.kernel_stats(15)[1] == 1
    w[17] = d["w"][17]
    eng.particles_upload(x, v, p, w)
    raw = eng.ptcldist(0, finish=False)
    ref = dx.exact(x, v, p, w, eng.local_sizes()[1], inp.lx, inp.v_max, 64, 65, 1, amd.diag_quanta(inp, 0))
    for k in PLANES:
        assert np.array_equal(raw[k], ref["raw"][k]), k
    assert np.array_equal(eng.energy_sums(0), ref["sums"])
    assert eng.kernel_stats(15)[1] == 1


def test_state_rules(amd):
    inp, eng = make(amd, n=400_001, nx=1024)
    pk = eng.predict_kind()
    eng.particle_load()
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    eng.interaction_push_particle(1)
    with pytest.raises(amd.Pic1dpError) as ex:
        eng.set_diag_sum(1)
    assert ex.value.code == 4          # PIC1DP_ERR_STATE
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    eng.interaction_push_particle(2)
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    with pytest.raises(amd.Pic1dpError):
        eng.set_diag_sum(2)
    with pytest.raises(amd.Pic1dpError):
        eng.diag_local_exact(0)        # kind 0 has no limbs
    eng.set_diag_sum(1)
    eng.set_output_fusion(2)           # ignored while kind 1 is set: the diagnostics keep their own pass
    passes = eng.kernel_stats(5)[1]
    eng.step(2)
    a = diagnostics(eng, 1)
    assert eng.kernel_stats(5)[1] == passes + 1
    assert eng.predict_kind() == pk    # the prediction of charge kind 0 survives
    eng.step(1)
    assert eng.predict_kind() == pk
    assert a["scal"][0] == pytest.approx(2 * inp.dt)
    eng.check_state(True)
    eng.set_diag_sum(0)
    eng.set_output_fusion(0)
    eng.check_state(True)
