"""The diagnostics pass of output_all (k_ptcldist) against the exact host reference (tests/diag_reference.py): bit for
bit on crafted edge markers, within rigorous bounds at 2^24 + 2^20 + 3 markers (the non-temporal variants, rows drawn
from the LDS counter), fixed-point and double sums; and the pass's division (diag_div) against IEEE division."""
import numpy as np
import pytest

import diag_reference as dr

pytestmark = pytest.mark.gpu

LX_DEFAULT = 2.0 * 3.1415926535897932384626 / 0.36
GRIDS = [(64, 64), (3, 2), (7, 5), (16, 200), (40, 200)]    # (40 x 200: beyond the LDS, the global-atomic path)
GEOMS = [(LX_DEFAULT, 8.0), (17.0, 10.0), (1.0 / 3.0, 7.3)]
NUM_CU = 256                       # MI355X: the pass launches min(256, the workgroups the markers fill) on the LDS path
N_SCALE = (1 << 24) + (1 << 20) + 3


def lds_path(nxo, nvo):
    return 8 * (3 * nxo * nvo + 3 * nvo) <= 150 * 1024


def vkey(k, lds):
    """the reference plane a v histogram of the pass compares with: the LDS path forms it as row sums"""
    return k.replace("_v", "_vrow") if lds and k.endswith("_v") else k


def engine(amd, n, lx, v_max, nxo, nvo, deltaf, **kw):
    kw = dict(nparticle_max=n, lx=lx, v_max=v_max, nx_opd=nxo, nv_opd=nvo, deltaf=deltaf, nx=64, **kw)
    if not deltaf:
        kw.update(iptcldist=0, species_density=[1.0], species_v0=[0.0])
    return amd.Pic1dp(amd.make_input(**kw))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("geom", GEOMS, ids=["lx_default-v8", "lx17-v10", "lx_third-v7.3"])
def test_diag_division_is_ieee(probe, geom, grid):
    """diag_div (reciprocal + two FMA corrections; the hardware division below 2^-500) against the IEEE quotient on 1e8
    dividends: positions with the cell boundaries +- ulps, 0 and subnormals, v + v_max with the bin boundaries +- ulps
    and the last ulps inside +-v_max"""
    lx, v_max = geom
    assert probe.diag_div_mismatches(lx, grid[0], v_max, grid[1], 20_000_000, 31) == 0      # 1e8 per (lx, v_max)
    assert probe.diag_div_mismatches(lx, grid[0], v_max, grid[1], 1_000_000, 31, host=True) == 0


# ---------------------------------------------------------------------------------------------------------------------
def padded(na, lx, v_max, x, v, p, w, idx):
    """na slots: the markers idx of (x, v, p, w) first, the rest at v = v_max (outside the histograms, inside the kinetic
    sums)"""
    X, V = np.full(na, 0.5 * lx), np.full(na, v_max)
    P, W = np.full(na, 0.75), np.full(na, -0.5)
    m = len(idx)
    X[:m], V[:m], P[:m], W[:m] = x[idx], v[idx], p[idx], w[idx]
    return X, V, P, W


@pytest.mark.parametrize("deltaf", [1, 0], ids=["deltaf", "fullf"])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("geom", GEOMS, ids=["lx_default-v8", "lx17-v10", "lx_third-v7.3"])
def test_edge_markers_bit_for_bit(amd, geom, grid, deltaf):
    """crafted markers (x = 0, 5e-324, the cell boundaries +- 1, 2 ulps, lx - ulp, lx; v = -v_max, -v_max + ulp, the bin
    boundaries +- ulps, +-0, v_max - 1..4 ulps, the top-row velocities, +-v_max) uploaded in batches that share no v row:
    every bin then holds one marker's terms, and the double pass equals the reference term for term -- raw, finished,
    through output_all; the kinetic sums over every slot; the next pass (fixed point on the LDS path) within its bound"""
    lx, v_max = geom
    nxo, nvo = grid
    lds = lds_path(nxo, nvo)
    x, v, p, w = dr.edge_markers(lx, v_max, nxo, nvo)
    eng = engine(amd, 64, lx, v_max, nxo, nvo, deltaf)
    na = eng.local_sizes()[0]
    groups = dr.batches(x, v, lx, v_max, nxo, nvo)
    assert max(len(g) for g in groups) <= na
    for gi, g in enumerate(groups):
        X, V, P, W = padded(na, lx, v_max, x, v, p, w, g)
        eng.particles_upload(X, V, P, W)
        ref = dr.reference(X, V, P, W, lx, v_max, nxo, nvo, deltaf, e_min=-1074)
        raw = eng.ptcldist(0, finish=False)
        for k in dr.PLANES:
            want = ref[vkey(k, lds)]["value"]
            assert np.array_equal(raw[k], want), (gi, k, np.flatnonzero(raw[k] != want)[:4])
        fin = eng.ptcldist(0, finish=True)
        want = eng.ptcldist_finish(raw)
        _, _, per = eng.output_all()
        for k in dr.PLANES:
            assert np.array_equal(fin[k], want[k]) and np.array_equal(per[0][k], want[k]), (gi, k)
        sums = eng.energy_sums(0)
        for k in range(3 if deltaf else 2):
            kin = ref["kinetic"][k]
            assert dr.error([sums[k]], kin)[0] <= dr.double_bound(kin, 2 * NUM_CU, 16)[0], (gi, k)
        if gi == 0:
            assert eng.kernel_stats(12)[1] == 0
    if not lds:
        return
    # the pass after the first one has its bounds: 64-bit fixed-point sums (the deposit bumps the marker state; its
    # wrap stores x == lx back as 0, hence the reference of the markers as they are now)
    eng.interaction_collect_charge()
    raw = eng.ptcldist(0, finish=False)
    assert eng.kernel_stats(12) == (0.0, 1)
    g = eng.particles_download()
    ref = dr.reference(g["x"], g["v"], g["p"], g["w"], lx, v_max, nxo, nvo, deltaf)
    q, blocks = dr.dist_quanta(na, NUM_CU, deltaf, 2.0 * np.max(np.abs(g["p"])), 16.0 * np.max(np.abs(g["w"])))
    for j, k in enumerate(dr.PLANES):
        if not deltaf and j % 3 == 2:
            continue
        plane = ref[vkey(k, lds)]
        assert np.all(dr.error(raw[k], plane) <= dr.fixed_bound(plane, q[j % 3], blocks)), k
        assert np.all(dr.on_grid(raw[k], q[j % 3])), k


# ---------------------------------------------------------------------------------------------------------------------
# What the library does not expose, the scale tests take from its rules: the non-temporal variants run where
# 32 np > 288 MiB (kernels_diag.hip launch_ptcldist; PIC1DP_DIAG_NT is a tuning-build knob, unset here), the LDS path
# where the histograms fit 150 KiB (lds_path), and the launch is min(256 CUs, the workgroups the markers fill).  Which
# pass summed in fixed point is counted by kernel_stats(12); that the step kernel took the diagnostics, by kernel_stats(5)
# (no k_ptcldist pass) and the name of the k_step_full instantiation launched last.
SCALE_INPUTS = {
    "bump": dict(),
    "maxwellian": dict(deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0]),
    "wide": dict(nx_opd=40, nv_opd=200),
    "two_species": dict(nspecies=2, species_charge=[-1.0, 1.0], species_mass=[1.0, 4.0], species_temperature=[1.0, 1.0],
                        species_temperature2=[1.0, 1.0], species_density=[0.9, 0.9], species_v0=[5.0, 5.0],
                        species_nparticle_init=[N_SCALE, (1 << 22) + 5]),
}


def scale_input(amd, key):
    return amd.make_input(nparticle_max=N_SCALE, nx=64, **SCALE_INPUTS[key])


def species_reference(g, na, npv, inp):
    """the reference of one species: histograms of its np markers, kinetic sums over all its slots (VecSum sums the
    whole local vector; slots beyond np hold what the load left there)"""
    ref = dr.reference(g["x"][:npv], g["v"][:npv], g["p"][:npv], g["w"][:npv], inp.lx, inp.v_max, inp.nx_opd, inp.nv_opd,
                       inp.deltaf)
    if npv < na:        # (v_max = 0: no tail slot enters the histograms)
        tail = dr.reference(g["x"][npv:], g["v"][npv:], g["p"][npv:], g["w"][npv:], inp.lx, 0.0, inp.nx_opd, inp.nv_opd,
                            inp.deltaf)
        ref["kinetic"] = [dr.combine(k, t) for k, t in zip(ref["kinetic"], tail["kinetic"])]
    return ref


@pytest.fixture(scope="module")
def scale(amd, request):
    """one particle_load of N_SCALE markers per input (request.param, a key of SCALE_INPUTS): the engine that loaded
    them (no pass has seen them yet), the markers per species as downloaded, and their exact references.  Module scope
    and indirect parametrisation: the tests of one input share them, and they are released before the next input"""
    inp = scale_input(amd, request.param)
    eng = amd.Pic1dp(inp)
    eng.particle_load()
    out = dict(eng=eng, inp=inp, g=[], ref=[], np=[])
    for s in range(inp.nspecies):
        na, npv = eng.local_sizes(s)
        g = eng.particles_download(s)
        out["g"].append(g)
        out["np"].append(npv)
        out["ref"].append(species_reference(g, na, npv, inp))
    yield out
    eng.close()


def compare(raw, ref, inp, fixed, tag, one):
    """every bin within its bound; prints max error / bound and the smallest bound / contribution of marker `one`"""
    nxo = inp.nx_opd
    lds = lds_path(nxo, inp.nv_opd)
    q, blocks = fixed if fixed else (None, 2 * NUM_CU)
    worst, sens = 0.0, np.inf
    for j, k in enumerate(dr.PLANES):
        if not inp.deltaf and j % 3 == 2:
            continue
        plane = ref[vkey(k, lds)]
        if fixed:
            bound = dr.fixed_bound(plane, q[j % 3], blocks)
            assert np.all(dr.on_grid(raw[k], q[j % 3])), (tag, k)
        else:
            bound = dr.double_bound(plane, blocks, nxo if lds and k.endswith("_v") else 0)
        err = dr.error(raw[k], plane)
        assert np.all(err <= bound), (tag, k, float(np.max(err - bound)))
        worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
        c = np.abs(one[vkey(k, lds)]["value"])
        if j % 3 == 0:        # sensitivity: dropping this marker moves its largest bins by >= 100x their bound
            hit = c > 0
            sens = min(sens, float(np.min(bound[hit] / c[hit])))
    assert sens <= 0.01, (tag, sens)
    print("%s: max error / bound %.3g; bound / the marker's largest contribution %.3g" % (tag, worst, sens))


def check_sums(eng, refs, tag):
    sums = []
    for s, ref in enumerate(refs):
        e = eng.energy_sums(s)
        for k in range(3 if eng.inp.deltaf else 2):
            kin = ref["kinetic"][k]
            assert dr.error([e[k]], kin)[0] <= dr.double_bound(kin, 2 * NUM_CU + 64, 16)[0], (tag, s, k)
        sums += list(e)
    assert np.array_equal(eng.output_scalars(), eng.output_scalars_from(np.array(sums))), tag


def one_marker(g, inp, i):
    return dr.reference(g["x"][i:i + 1], g["v"][i:i + 1], g["p"][i:i + 1], g["w"][i:i + 1],
                        inp.lx, inp.v_max, inp.nx_opd, inp.nv_opd, inp.deltaf)


def quanta(g, npv, inp, margin_w=16.0):
    """the fixed-point quanta of a pass whose bounds came from a pass over the markers g (2 max |p|, margin max |w|)"""
    return dr.dist_quanta(npv, NUM_CU, inp.deltaf, 2.0 * np.max(np.abs(g["p"][:npv])),
                          margin_w * np.max(np.abs(g["w"][:npv])))


def two_passes(eng, sc, tag, expect_fixed):
    """first pass per species (bounds unknown: doubles), then a second on the same markers (fixed point where
    expected), output_all's record of it, the kinetic sums"""
    inp, ns = sc["inp"], sc["inp"].nspecies
    fx0 = eng.kernel_stats(12)[1]
    ones = [one_marker(sc["g"][s], inp, sc["np"][s] - 1) for s in range(ns)]   # (odd np: the first workgroup's thread 0)
    for s in range(ns):
        compare(eng.ptcldist(s, finish=False), sc["ref"][s], inp, None, "%s species %d pass 1 (double)" % (tag, s), ones[s])
    assert eng.kernel_stats(12)[1] == fx0
    check_sums(eng, sc["ref"], tag)
    eng.interaction_collect_charge()                     # (state bumped; x of a load already lies in [0, lx))
    raws = []
    for s in range(ns):
        raw = eng.ptcldist(s, finish=False)
        fixed = quanta(sc["g"][s], sc["np"][s], inp) if expect_fixed else None
        compare(raw, sc["ref"][s], inp, fixed, "%s species %d pass 2 (%s)" % (tag, s, "fixed point" if fixed else "double"),
                ones[s])
        raws.append(raw)
    assert eng.kernel_stats(12) == (0.0, fx0 + (ns if expect_fixed else 0))
    _, _, per = eng.output_all()
    for s in range(ns):
        want = eng.ptcldist_finish(raws[s], s)
        for k in dr.PLANES:
            assert np.array_equal(per[s][k], want[k]), (tag, s, k)
    check_sums(eng, sc["ref"], tag)


def uploaded(amd, sc):
    eng = amd.Pic1dp(sc["inp"])
    g = sc["g"][0]
    eng.particles_upload(g["x"], g["v"], g["p"], g["w"], np_valid=sc["np"][0])
    return eng


N_ROWS = (1 << 18) + 3


@pytest.fixture(scope="module")
def rows_case(amd):
    """N_ROWS loaded markers of the default case and their reference, once"""
    inp = amd.make_input(nparticle_max=N_ROWS, nx=64)
    with amd.Pic1dp(inp) as eng:
        eng.particle_load()
        na, npv = eng.local_sizes(0)
        g = eng.particles_download(0)
    return inp, g, npv, species_reference(g, na, npv, inp), one_marker(g, inp, npv - 1)


@pytest.mark.parametrize("drawn", ["0", "16"])
def test_rows_all_dealt_and_all_drawn(amd, monkeypatch, tuning, rows_case, drawn):
    """tuning knob PIC1DP_DYN_TAIL at its two ends -- every row of a workgroup dealt, every row drawn by its waves: the
    histograms of the double pass and the kinetic sums within the bounds of the default setting"""
    inp, g, npv, ref, one = rows_case
    monkeypatch.setenv("PIC1DP_DYN_TAIL", drawn)
    with amd.Pic1dp(inp) as eng:
        eng.particles_upload(g["x"], g["v"], g["p"], g["w"], np_valid=npv)
        compare(eng.ptcldist(0, finish=False), ref, inp, None, "PIC1DP_DYN_TAIL=%s (double)" % drawn, one)
        assert eng.kernel_stats(12)[1] == 0
        check_sums(eng, [ref], "PIC1DP_DYN_TAIL=%s" % drawn)


@pytest.mark.parametrize("scale", ["bump"], indirect=True)
def test_scale_deltaf_bump_on_tail(amd, scale, monkeypatch):
    """(a) delta f bump-on-tail, default geometry: the double pass, the fixed-point pass, output_all -- on the engine
    that loaded the markers; (b) the same markers uploaded into an engine with PIC1DP_DIAG_FX=0: both passes in doubles"""
    assert 32.0 * N_SCALE > 288.0 * 1048576.0 and lds_path(64, 64)
    two_passes(scale["eng"], scale, "(a) bump-on-tail", True)
    monkeypatch.setenv("PIC1DP_DIAG_FX", "0")
    with uploaded(amd, scale) as eng:
        two_passes(eng, scale, "(b) PIC1DP_DIAG_FX=0", False)
        assert eng.kernel_stats(12) == (0.0, 0)


@pytest.mark.parametrize("scale", ["bump"], indirect=True)
def test_scale_overflowing_fixed_point_pass_repeats_in_doubles(amd, scale, monkeypatch):
    """(g) PIC1DP_DIAG_FX_MARGIN=0.5: the second pass's bound on |w| is half the largest |w|, the fixed-point pass
    overflows and is repeated in doubles"""
    monkeypatch.setenv("PIC1DP_DIAG_FX_MARGIN", "0.5")
    inp, ref = scale["inp"], scale["ref"][0]
    with uploaded(amd, scale) as eng:
        one = one_marker(scale["g"][0], inp, 12345)
        compare(eng.ptcldist(0, finish=False), ref, inp, None, "(g) pass 1", one)
        eng.interaction_collect_charge()
        raw = eng.ptcldist(0, finish=False)
        assert eng.kernel_stats(12) == (1.0, 1)          # one fixed-point pass, repeated in doubles
        compare(raw, ref, inp, None, "(g) pass 2 (repeated in doubles)", one)
        check_sums(eng, scale["ref"], "(g)")


@pytest.mark.parametrize("scale", ["bump"], indirect=True)
def test_scale_diagnostics_inside_the_step_kernel(amd, scale):
    """(f) output fusion: the step before output_all takes the diagnostics inside k_step_full<DIAG> (its own drawn-chunk
    loop and non-temporal loads), in fixed point with the bounds of a pass before it; against the reference of the
    markers that step left"""
    inp = scale["inp"]
    g0 = scale["g"][0]
    with uploaded(amd, scale) as eng:
        eng.ptcldist(0, finish=False)                    # the pass whose max |p|, |w| scale the step's fixed-point sums
        eng.set_output_fusion(2)
        eng.interaction_collect_charge()
        eng.field_solve_electric()
        eng.kernel_stats_enable(True)
        passes = eng.kernel_stats(5)[1]                  # k_ptcldist passes so far (the one above)
        eng.step(10)                                     # dt 0.05, output_interval 0.5: the tenth step precedes output_all
        assert eng.output_due()
        assert "k_step_full<DIAG>" in eng.kernel_bytes(4)["name"]
        raw = eng.ptcldist(0, finish=False)
        assert eng.kernel_stats(5)[1] == passes          # no k_ptcldist pass: the step kernel's diagnostics
        assert eng.kernel_stats(12) == (0.0, 1)          # ... summed in fixed point, no repeat
        g = eng.particles_download()
        ref = dr.reference(g["x"], g["v"], g["p"], g["w"], inp.lx, inp.v_max, inp.nx_opd, inp.nv_opd, inp.deltaf)
        assert not np.array_equal(g["x"], g0["x"])
        compare(raw, ref, inp, quanta(g0, N_SCALE, inp), "(f) k_step_full<DIAG> (fixed point)", one_marker(g, inp, N_SCALE - 1))
        check_sums(eng, [ref], "(f)")
        assert eng.kernel_stats(5)[1] == passes


@pytest.mark.parametrize("scale", ["maxwellian"], indirect=True)
def test_scale_fullf_maxwellian(scale):
    """(c) full f, Maxwellian"""
    two_passes(scale["eng"], scale, "(c) full-f Maxwellian", True)


@pytest.mark.parametrize("scale", ["wide"], indirect=True)
def test_scale_global_atomic_path(scale):
    """(d) 40 x 200: histograms too large for the LDS, double atomics straight into the output (16 x 200 still fits);
    the global-atomic path has no fixed-point variant, so both passes sum in doubles"""
    assert lds_path(16, 200) and not lds_path(40, 200)
    two_passes(scale["eng"], scale, "(d) 40x200", False)


@pytest.mark.parametrize("scale", ["two_species"], indirect=True)
def test_scale_two_species_of_unequal_counts(scale):
    """(e) two species, 2^24 + 2^20 + 3 and 2^22 + 5 markers (the first takes the non-temporal variants, the second not):
    each species' histograms, partial sums and fixed-point bounds against its own reference"""
    assert scale["np"] == [N_SCALE, (1 << 22) + 5]
    assert 32.0 * scale["np"][1] <= 288.0 * 1048576.0
    two_passes(scale["eng"], scale, "(e) two species", True)


def test_two_species_overflow_repeats_through_the_separate_calls(amd, monkeypatch):
    """(h) the repeat in doubles as energy_sums / ptcldist reach it (the collector's other caller: output_all has
    test_output_all_record_survives_a_fixed_point_repeat), two species of 4097 and 2049 markers (one workgroup each, an
    odd last marker), 16 x 16 bins, PIC1DP_DIAG_FX_MARGIN=0.5: each species' second pass overflows its bound on |w| and
    is repeated; the repeat of one species leaves the other's cached sums and histograms alone"""
    monkeypatch.setenv("PIC1DP_DIAG_FX_MARGIN", "0.5")
    counts = [4097, 2049]
    inp = amd.make_input(nparticle_max=counts[0], nx=64, nx_opd=16, nv_opd=16,
                         **dict(SCALE_INPUTS["two_species"], species_nparticle_init=counts))
    with amd.Pic1dp(inp) as eng:
        eng.particle_load()
        g = [eng.particles_download(s) for s in range(2)]
        sizes = [eng.local_sizes(s) for s in range(2)]
        assert [npv for _, npv in sizes] == counts
        refs = [species_reference(g[s], sizes[s][0], counts[s], inp) for s in range(2)]
        ones = [one_marker(g[s], inp, counts[s] - 1) for s in range(2)]
        for s in range(2):
            compare(eng.ptcldist(s, finish=False), refs[s], inp, None, "(h) species %d pass 1" % s, ones[s])
        assert eng.kernel_stats(12) == (0.0, 0)
        eng.interaction_collect_charge()
        e0 = eng.energy_sums(0)                          # species 0: the overflow met by energy_sums
        assert eng.kernel_stats(12) == (1.0, 1)
        raw1 = eng.ptcldist(1, finish=False)             # species 1: by ptcldist
        assert eng.kernel_stats(12) == (2.0, 2)          # two fixed-point passes, each repeated in doubles
        raw0 = eng.ptcldist(0, finish=False)             # (cached: no further pass)
        assert eng.kernel_stats(12) == (2.0, 2) and np.array_equal(eng.energy_sums(0), e0)
        compare(raw0, refs[0], inp, None, "(h) species 0 pass 2 (repeated in doubles)", ones[0])
        compare(raw1, refs[1], inp, None, "(h) species 1 pass 2 (repeated in doubles)", ones[1])
        check_sums(eng, refs, "(h)")
