"""The on-device particle load on the GPU: k_load against tests/load_reference.py -- x and v bit for bit,
p and w inside a bound derived from the operation count --, the index function beyond 2^32, independence of the rank
layout, the digest without a download, the steps, events and checkpoint after it, what a quiet start buys, the refusals."""
import os
import subprocess

import numpy as np
import pytest

import load_reference as R
from test_gpu_output import fortran_host_exe
from test_gpu_parity import assert_w_close, assert_w_close_one_exp, one_exp_active, w_cancellation
from util import ulp_diff

pytestmark = pytest.mark.gpu

U = 2.0 ** -53                      # unit roundoff of a double
ERR_ARG = 1
TWO = dict(nspecies=2, species_charge=[-1.0, 1.0], species_mass=[1.0, 4.0], species_temperature=[1.0, 1.0],
           species_temperature2=[1.0, 1.0], species_density=[0.9, 0.9], species_v0=[5.0, 5.0])
DISTS = [dict(), dict(iptcldist=0, species_density=[1.0], species_v0=[0.3], species_temperature=[1.7], species_mass=[0.9]),
         dict(iptcldist=1, species_density=[1.0]),
         dict(iptcldist=2, species_density=[1.0], species_v0=[3.0], species_temperature=[0.9], species_mass=[1.2])]


def dev(amd, kind, rank=0, nranks=1, npe=0, seed_offset=0, host_first=False, **kw):
    kw.setdefault("nx", 64)
    e = amd.Pic1dp(amd.make_input(**kw), rank=rank, nranks=nranks, npe=npe, device=0)
    if host_first:      # the host load fills the tail slots with markers: the device load has something to overwrite
        e.particle_load()
    if seed_offset:
        e.set_seed_offset(seed_offset)
    e.particle_load_device(kind)
    return e


def valid(e, s=0):
    npv = e.local_sizes(s)[1]
    return {k: a[:npv] for k, a in e.particles_download(s).items()}


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def check_species(e, kind, s=0, g0=0, seed_offset=0):
    """x, v bit for bit; the tail +0.0 in all four arrays; p, w inside the bound.

    The bound, in units of u = 2^-53, from the kernel's operation count against a reference that evaluates the same
    formula on the same x and v in extended precision (error ~1e-19, neglected).  With A the marker's largest |argument|
    of an exp and f its unperturbed weight:
      exp: pexp lies within 1 ulp = 2u of libm, libm within 1 ulp = 2u of the true value; its argument carries the
           rounding of v -+ v0 twice in the square (2u), of the square (u), of the division (u) and of the host's
           constant 2T/m (u): 5u A relative in the exponential                                      -> (4 + 5 A) u
      a term: times density (u), over its norm (u), the norm itself a rounded sqrt of two rounded products (2u) -> 4u
      the sum of the (positive) terms (u), times the prefactor (u), the prefactor three rounded operations (3u) -> 5u
      |f - f_ref| <= (13 + 5 A) u f.
    amp = sum_j (c_j cos + s_j sin) over the init modes, the argument k_j x the same double on both sides: sincos within
    4 ulp = 8u (the OpenCL bound for double, which the device library meets), each product (u) and each of the 2 n_j
    additions (u) on terms of at most S = sum_j |c_j| + |s_j|:   |amp - amp_ref| <= (9 + 2 n_j) u S.
      |w - w_ref| <= [(9 + 2 n_j) S + (14 + 5 A) |amp|] u f      (w = amp f: both errors and the product's rounding)
      |p - p_ref| <= the bound on f, plus in a nonlinear run the bound on w and u |p| for the addition."""
    inp = e.inp
    nalloc, npv = e.local_sizes(s)
    got = e.particles_download(s)
    ref = R.markers(inp, kind, s, g0, npv, seed_offset)
    for k in "xv":
        assert same_bits(got[k][:npv], ref[k]), (k, s)
    for k in "xvpw":
        assert same_bits(got[k][npv:], np.zeros(nalloc - npv)), (k, s, "tail")
    L = np.longdouble
    nj = inp.init_nmode
    S = L(sum(abs(inp.init_mode_cos[j]) + abs(inp.init_mode_sin[j]) for j in range(nj)))
    f, A = ref["f"], ref["arg"]
    bf = (13 + 5 * A) * U * f
    bw = ((9 + 2 * nj) * S + (14 + 5 * A) * np.abs(ref["amp"])) * U * f
    bp = bf + (bw + U * np.abs(ref["p"]) if inp.linear == 0 else 0)
    tiny = L(np.finfo(np.float64).tiny)           # (below the normal range an ulp is no longer relative: none occurs here)
    for k, b in (("p", bp), ("w", bw)):
        err = np.abs(got[k][:npv].astype(L) - ref[k])
        ratio = float(np.max(err / np.maximum(b, tiny))) if npv else 0.0
        print("load kind %d dist %d species %d n %d: worst |%s error| / bound = %.3f" % (kind, inp.iptcldist, s, npv, k, ratio))
        assert np.all(err <= np.maximum(b, tiny)), (k, s, ratio)
    return got


# ---------------------------------------------------------------------------
# 1. + 2. bits of x and v, the tail, p and w
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, 2 * 4096 + 1, 100_001])
def test_markers_equal_the_restatement(amd, kind, n):
    e = dev(amd, kind, nparticle_max=n)
    check_species(e, kind)
    assert e.kernel_stats(19)[1] == 1 and e.itime == 0 and e.time == 0.0
    e.close()


@pytest.mark.parametrize("kind", [1, 2])
def test_fewer_markers_than_slots_two_species_and_a_linear_run(amd, kind):
    e = dev(amd, kind, host_first=True, nparticle_max=9000, species_nparticle_init=[4097, 8191], **TWO)
    assert e.local_sizes(0) == (9000, 4097) and e.local_sizes(1) == (9000, 8191)
    g = [check_species(e, kind, s) for s in (0, 1)]
    assert e.kernel_stats(19)[1] == 2
    if kind == 2:     # one sequence for every species: co-located markers
        assert same_bits(g[0]["x"][:4097], g[1]["x"][:4097]) and same_bits(g[0]["v"][:4097], g[1]["v"][:4097])
    else:
        assert not np.any(g[0]["x"][:4097] == g[1]["x"][:4097])
    e.close()
    lin = dev(amd, kind, nparticle_max=4099, species_nparticle_init=[4098], linear=1, iptcldist=0, species_density=[1.0],
              species_v0=[0.0])
    got = check_species(lin, kind)
    non = dev(amd, kind, nparticle_max=4099, species_nparticle_init=[4098], linear=0, iptcldist=0, species_density=[1.0],
              species_v0=[0.0])
    gn = non.particles_download()
    assert same_bits(got["w"], gn["w"]) and same_bits(got["p"] + got["w"], gn["p"])      # p += w in the nonlinear run only
    assert np.any(gn["p"] != got["p"])
    lin.close(), non.close()


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("dist", range(4))
def test_every_distribution(amd, kind, dist):
    e = dev(amd, kind, nparticle_max=2 * 4096 + 3, init_nmode=2, init_mode=[1, 3], init_mode_cos=[1e-3, 0.0],
            init_mode_sin=[2e-4, 5e-4], nmode=3, modes=[1, 2, 3], **DISTS[dist])
    check_species(e, kind)
    e.close()


@pytest.mark.parametrize("kind", [1, 2])
def test_three_reference_blocks_in_one_context_and_a_seed_offset(amd, kind):
    e = dev(amd, kind, npe=3, nparticle_max=10_007, species_nparticle_init=[10_001])
    check_species(e, kind)          # the blocks' valid markers are contiguous: global markers 0 ... N - 1
    e.close()
    if kind == 1:
        m = dev(amd, 1, seed_offset=3, nparticle_max=4097)
        check_species(m, 1, seed_offset=3)
        m.close()


# ---------------------------------------------------------------------------
# 3. the index function beyond 2^32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 2])
def test_device_index_function_beyond_two_to_the_32(amd, probe, kind):
    g = np.array([0, 1, 2**32 - 1, 2**32, 2**33 + 5, 3**21 - 1], dtype=np.int64)
    for s in (0, 1):
        uv, ux = probe.load_uniforms(kind, g, ispecies=s)
        for i, gi in enumerate(g):
            huv, hux = amd.load_uniforms(kind, int(gi), 1, ispecies=s)
            assert same_bits(uv[i], huv[0]) and same_bits(ux[i], hux[0]), (kind, int(gi))
    # and a dense run across the split of the base-3 reversal (3^10 and its multiples) and across 2^32
    for g0 in (3**10 - 8, 7 * 3**10 - 8, 2**32 - 8, 3**20 - 8):
        gg = np.arange(g0, g0 + 16, dtype=np.int64)
        uv, ux = probe.load_uniforms(kind, gg)
        huv, hux = amd.load_uniforms(kind, g0, 16)
        assert same_bits(uv, huv) and same_bits(ux, hux), (kind, g0)


# ---------------------------------------------------------------------------
# 4. the same markers whatever the layout
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 2])
def test_markers_do_not_depend_on_the_rank_layout(amd, kind):
    kw = dict(nparticle_max=3 * 4096 + 5, nx=64)
    one = dev(amd, kind, **kw)
    four = dev(amd, kind, npe=4, **kw)
    two = [dev(amd, kind, rank=r, nranks=2, **kw) for r in range(2)]
    ref = valid(one)
    assert ref["x"].size == 3 * 4096 + 5
    parts = [valid(e) for e in two]
    assert parts[0]["x"].size == amd.load_origin(one.inp, 0, rank=1, nranks=2) > 0
    for k in "xvpw":
        assert same_bits(valid(four)[k], ref[k]), k
        assert same_bits(np.concatenate([p[k] for p in parts]), ref[k]), k
    for e in [one] + two:
        e.set_charge_sum(1)
    want = one.charge_local_exact()
    got = two[0].charge_local_exact() + two[1].charge_local_exact()
    as_int = lambda a: [int(h) * 2**32 + int(l) for h, l in zip(a[0, 0], a[0, 1])]
    assert as_int(got) == as_int(want) and any(as_int(want))
    for e in [one, four] + two:
        e.close()


# ---------------------------------------------------------------------------
# 5. without a download
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 2])
def test_digest_of_four_million_markers_equals_the_restatements(amd, kind):
    n = 2**22 + 3
    e = dev(amd, kind, nparticle_max=n + 2, species_nparticle_init=[n])
    x, v = R.xv(e.inp, kind)
    tail = np.zeros(2)
    d = e.state_digest()
    assert int(d[0][0]) == amd.host_digest(np.concatenate([x, tail])) and int(d[0][1]) == amd.host_digest(np.concatenate([v, tail]))
    e.close()


def test_reload_after_steps_and_host_load_after_a_device_load(amd):
    kw = dict(nparticle_max=20_001, nx=64)
    fresh = dev(amd, 2, **kw)
    want = fresh.state_digest().tolist()
    e = dev(amd, 1, **kw)
    e.interaction_collect_charge()
    e.field_solve_electric()
    e.step(5)
    e.particle_load_device(2)
    assert e.state_digest().tolist() == want and e.itime == 0 and e.energy_history().size == 0
    host = amd.Pic1dp(amd.make_input(**kw))
    host.particle_load()
    e.particle_load()
    assert e.state_digest().tolist() == host.state_digest().tolist()
    for x in (fresh, e, host):
        x.close()


# ---------------------------------------------------------------------------
# 6. the step after it
# ---------------------------------------------------------------------------
STEPS_KW = dict(nparticle_max=20_001, nx=64, nmode=2, modes=[1, 2])


def oracle_with_the_markers_of(oracle_mod, e, **kw):
    sim = oracle_mod.Sim(oracle_mod.make_input(**kw))
    assert sim.load() == 0
    g = e.particles_download()
    for k in "xvpw":
        sim.array(0, 0, k)[:] = g[k]
    return sim


@pytest.mark.parametrize("kind", [1, 2])
def test_call_sites_after_a_device_load_on_the_oracles_field(oracle_mod, amd, probe, kind):
    """The device-loaded markers copied into the oracle, 20 steps through the call sites, both sides pushed by ONE field: the
    engine's solve is handed to the oracle before every sub-step (its own differs by the order of the charge sums, 1e-13).
    After every push x and v are equal bit for bit, p too, and w lies within the push's own bound (tests/test_gpu_parity.py
    test_push_particle: the device's exp against libm's and the conditioning of -f0'/f0 -- the only operation of a push that
    is not the same IEEE operation on both sides); the oracle then takes the engine's w, so the bound is per push, not summed.
    The energy of every solve stays within 1e-10 of the oracle's own."""
    e = dev(amd, kind, **STEPS_KW)
    sim = oracle_with_the_markers_of(oracle_mod, e, **STEPS_KW)
    one_exp = one_exp_active(probe, sim.inp)
    p0 = e.particles_download()["p"]
    sim.collect_charge(), sim.solve_field()
    e.interaction_collect_charge(), e.field_solve_electric()
    for it in range(20):
        for irk in (1, 2):
            sim.set_field(e.get_field(chargeden=False)["electric"])
            wb = sim.gather("w") if irk == 1 else sim.gather("wb")
            v_at = sim.gather("v")
            sim.push(irk)
            e.interaction_push_particle(irk)
            g = e.particles_download()
            assert same_bits(g["x"], sim.gather("x")), ("x", it, irk)
            assert same_bits(g["v"], sim.gather("v")), ("v", it, irk)
            assert same_bits(g["p"], sim.gather("p")) and same_bits(g["p"], p0), ("p", it, irk)
            if one_exp:
                assert_w_close_one_exp(sim.inp, v_at, g["w"], sim.gather("w"), wb)
            else:
                assert_w_close(g["w"], sim.gather("w"), wb, False, w_cancellation(sim.inp, v_at))
            sim.array(0, 0, "w")[:] = g["w"]
            sim.collect_charge(), sim.solve_field()
            e.interaction_collect_charge(), e.field_solve_electric()
            assert abs(e.field_energy() / sim.field_energy() - 1.0) < 1e-10, (it, irk)
    e.close()


@pytest.mark.parametrize("kind", [1, 2])
def test_free_running_steps_after_a_device_load_follow_the_oracle(oracle_mod, amd, monkeypatch, kind):
    """... and left alone: 20 steps through step() and through the lazy call sites (nobody looks in between), each side on
    its own field.  The field energy of every step within 1e-10 of the oracle's.  The markers afterwards can no longer be
    bit-equal -- the fields differ by the order of the charge sums -- and are held to what a field within delta = 1e-10
    allows, with F = max |E| |Z/m| of the run and T = 20 dt:
      p: no step changes it: bit for bit;
      v: every sub-step adds dt E(x) Z/m: |dv| <= 4 delta T F (the field's delta at both sub-steps: 2; the gather at the
         displaced x and the interpolation weights: 2) plus 64 ulp of v_max for forty roundings;
      x: the suite's bar for such a run (test_gpu_parity.py test_run_two_species): 2^20 ulp;
      w: every step adds an update that is linear in E and smooth in x, v: |dw| <= 8 delta sum_n |w_(n+1) - w_n| (the sum
         taken from the oracle, step by step; field 2, gather 2, the factor p - w and -f0'/f0 at the displaced v 2) plus
         64 ulp of max |w|.
    The two GPU paths are held to the same bars against each other.  Two kept modes: the prediction tiles' fixed-point
    bounds the load seeded hold (kernel_stats 13 stays 0)."""
    kw = STEPS_KW
    runs = {}
    for path in ("step", "calls"):
        monkeypatch.setenv("PIC1DP_LAZY_CALLS", "1")
        e = dev(amd, kind, **kw)
        sim = oracle_with_the_markers_of(oracle_mod, e, **kw)
        sim.collect_charge(), sim.solve_field()
        e.interaction_collect_charge(), e.field_solve_electric()
        assert abs(e.field_energy() / sim.field_energy() - 1.0) < 1e-10
        eo, wsum, emax = [], np.zeros(sim.array(0, 0, "w").size), float(np.max(np.abs(sim.get_field()[0])))
        for _ in range(20):
            w0 = sim.array(0, 0, "w").copy()
            sim.step(1)
            wsum += np.abs(sim.array(0, 0, "w") - w0)
            emax = max(emax, float(np.max(np.abs(sim.get_field()[0]))))
            eo.append(sim.field_energy())
        if path == "step":
            e.step(20)
            eg = e.energy_history()
        else:
            eg = []
            for _ in range(20):
                for irk in (1, 2):
                    e.interaction_push_particle(irk)
                    e.particle_optimize(irk)
                    e.interaction_collect_charge()
                    e.field_solve_electric()
                eg.append(e.field_energy())
            eg = np.array(eg)
        assert eg.size == 20 and np.max(np.abs(eg / np.array(eo) - 1.0)) < 1e-10
        assert e.kernel_stats(13)[1] == 0
        got = e.particles_download()
        inp = e.inp
        eps = np.finfo(np.float64).eps
        F = emax * abs(inp.species_charge[0] / inp.species_mass[0])
        bars = dict(v=4 * 1e-10 * 20 * inp.dt * F + 64 * eps * inp.v_max,
                    w=8 * 1e-10 * wsum + 64 * eps * float(np.max(np.abs(sim.array(0, 0, "w")))))
        runs[path] = (got, bars)
        assert same_bits(got["p"], sim.array(0, 0, "p"))
        assert np.max(ulp_diff(got["x"], sim.array(0, 0, "x"))) <= 2**20
        for k in "vw":
            err = np.abs(got[k] - sim.array(0, 0, k))
            print("load kind %d, %s: worst |%s - oracle| / bar = %.3g" % (kind, path, k, float(np.max(err / np.maximum(bars[k], 1e-300)))))
            assert np.all(err <= bars[k]), (k, path)
        e.close()
    (a, bars), (b, _) = runs["step"], runs["calls"]
    assert np.max(ulp_diff(a["x"], b["x"])) <= 2**20 and same_bits(a["p"], b["p"])
    for k in "vw":
        assert np.all(np.abs(a[k] - b[k]) <= 2 * bars[k]), k


# ---------------------------------------------------------------------------
# 7. events and checkpoint
# ---------------------------------------------------------------------------
def test_split_event_after_a_device_load_runs_the_same_in_twin_contexts(amd):
    kw = dict(nparticle_max=60_000, species_nparticle_init=[36_000], nx=32, nv=64, nsplit=1, tsplit=[0.1], thshsplit=[0.3])
    twins = [dev(amd, 2, **kw) for _ in range(2)]
    for e in twins:
        e.set_charge_sum(1)
        e.interaction_collect_charge()
        e.field_solve_electric()
        e.step(4)
    assert twins[0].local_sizes(0)[1] > 36_000                  # the split has run
    assert twins[0].local_sizes(0) == twins[1].local_sizes(0)
    assert twins[0].state_digest().tolist() == twins[1].state_digest().tolist()
    for e in twins:
        e.close()


def test_checkpoint_after_a_quiet_start(amd, tmp_path):
    a = dev(amd, 2, nparticle_max=20_001, nx=64)
    a.set_charge_sum(1)
    a.interaction_collect_charge()
    a.field_solve_electric()
    a.step(3)
    path = str(tmp_path / "quiet.ckpt")
    a.checkpoint_write(path)
    b = amd.Pic1dp.from_checkpoint(path)
    a.step(3), b.step(3)
    assert a.state_digest().tolist() == b.state_digest().tolist()
    assert same_bits(a.energy_history(), b.energy_history()) and a.energy_history().size == 6
    a.close(), b.close()


# ---------------------------------------------------------------------------
# 8. what a quiet start is for
# ---------------------------------------------------------------------------
def _start(amd, kind, n):
    e = dev(amd, kind, nparticle_max=n, nx=64)
    e.interaction_collect_charge()
    e.field_solve_electric()
    return e


def test_quiet_start_is_quiet_and_its_growth_rate_converged(oracle_mod, amd):
    """default bump-on-tail input, nx 64.  The modes nobody excited (2 ... 8) of the deposited charge density: kind 2 at
    most a tenth of kind 1 at 2^16 markers; the initial field energy of kind 2 at 2^16 and 2^18 markers within 2e-4; the
    growth rate fitted over t in [20, 55) of 1 100 steps within 0.1 % between the two sizes and within 0.5 % of
    2 gamma = 0.1679723.  Kind 1 is logged beside it."""
    theory = 0.1679723
    out = {}
    for kind in (1, 2):
        for n in (2**16, 2**18):
            e = _start(amd, kind, n)
            cd = e.get_field()["chargeden"]
            amp = np.abs(np.fft.rfft(cd))[2:9] / cd.size
            e0 = e.field_energy()
            e.step(1100)
            en = np.concatenate([[e0], e.energy_history()])
            t = np.arange(en.size) * e.inp.dt
            rate = oracle_mod.growthrate_energy_fit(t, en, 20.0, 55.0)
            out[kind, n] = (float(amp.max()), e0, rate)
            print("load kind %d, %6d markers: modes 2..8 of chargeden <= %.3e, initial energy %.9e, 2 gamma %.6f (%+.2f %% of theory)"
                  % (kind, n, amp.max(), e0, rate, 100 * (rate / theory - 1)))
            e.close()
    print("quiet / random amplitude of the modes not excited at 2^16 markers: 1 / %.1f" % (out[1, 2**16][0] / out[2, 2**16][0]))
    print("quiet start, initial energy 2^16 against 2^18: %.2e relative" % abs(out[2, 2**16][1] / out[2, 2**18][1] - 1))
    print("quiet start, 2 gamma 2^16 against 2^18: %.3f %%" % (100 * abs(out[2, 2**16][2] / out[2, 2**18][2] - 1)))
    assert out[2, 2**16][0] <= out[1, 2**16][0] / 10
    assert abs(out[2, 2**16][1] / out[2, 2**18][1] - 1) <= 2e-4
    assert abs(out[2, 2**16][2] / out[2, 2**18][2] - 1) <= 1e-3
    for n in (2**16, 2**18):
        assert abs(out[2, n][2] / theory - 1) <= 5e-3


# ---------------------------------------------------------------------------
# 9. refusals leave the context alone
# ---------------------------------------------------------------------------
def test_refused_calls_leave_the_context_untouched(amd):
    e = dev(amd, 1, nparticle_max=4097)
    e.interaction_collect_charge()
    e.field_solve_electric()
    e.step(2)
    before, markers, it = e.state_digest().tolist(), e.particles_download(), e.itime
    for kind, word in ((0, "kind"), (3, "kind")):
        with pytest.raises(amd.Pic1dpError) as ei:
            e.particle_load_device(kind)
        assert ei.value.code == ERR_ARG and word in str(ei.value)
    e.set_seed_offset(2)
    with pytest.raises(amd.Pic1dpError) as ei:
        e.particle_load_device(2)
    assert ei.value.code == ERR_ARG and "seed offset" in str(ei.value)
    assert e.state_digest().tolist() == before and e.itime == it == 2 and e.energy_history().size == 2
    after = e.particles_download()
    assert all(same_bits(after[k], markers[k]) for k in "xvpw")
    assert e.kernel_stats(19)[1] == 1
    e.close()
    g = amd.Pic1dp(amd.make_input(nparticle_max=4097, imarker=1, iptcldist=0, species_density=[1.0], species_v0=[0.0]))
    g.particle_load()
    before = g.state_digest().tolist()
    for kind in (1, 2):
        with pytest.raises(amd.Pic1dpError) as ei:
            g.particle_load_device(kind)
        assert ei.value.code == ERR_ARG and "imarker" in str(ei.value)
    assert g.state_digest().tolist() == before and g.kernel_stats(19)[1] == 0
    g.close()


# ---------------------------------------------------------------------------
# 10. the Fortran host's PIC1DP_LOAD
# ---------------------------------------------------------------------------
def test_fortran_host_takes_its_load_from_the_environment(amd, tmp_path):
    """PIC1DP_LOAD=quiet and =random: the host's first record (the field of the loaded markers, exact charge sum: no order)
    and the p it dumps at the end equal those of particle_load_device(2) and (1) in a Python context, bit for bit, and differ
    from the host load's; a word that only begins like one of the three is refused."""
    exe = fortran_host_exe()
    from pic1dp_amd import output
    base = dict(os.environ, PIC1DP_NPARTICLE="4097", PIC1DP_NX="64", PIC1DP_TIME_MAX="0.1", PIC1DP_CHARGE_SUM="exact")
    for k in ("PIC1DP_LOAD", "PIC1DP_RANK", "PIC1DP_NRANKS", "PIC1DP_RESTART", "PIC1DP_CHECKPOINT_AT", "PIC1DP_FUSED"):
        base.pop(k, None)
    first = {}
    for word, kind in (("host", 0), ("quiet", 2), ("random", 1), (None, 0)):
        wd = tmp_path / str(word)
        wd.mkdir()
        env = dict(base, PIC1DP_DUMP_MARKERS=str(wd / "markers.bin"))
        if word:
            env["PIC1DP_LOAD"] = word
        r = subprocess.run([exe], cwd=str(wd), env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        m = np.fromfile(str(wd / "markers.bin"))
        assert int(m[0]) == 4097 and m.size == 1 + 4 * 4097
        rec = output.OutputData(str(wd / "pic1dp.out"))
        e = amd.Pic1dp(amd.make_input(nparticle_max=4097, nx=64))
        if kind:
            e.particle_load_device(kind)
        else:
            e.particle_load()
        e.set_charge_sum(1)
        e.interaction_collect_charge()
        e.field_solve_electric()
        assert same_bits(np.asarray(rec.electric[0]), e.get_field()["electric"]), word
        assert same_bits(m[1 + 2 * 4097:1 + 3 * 4097], e.particles_download()["p"]), word
        first[word] = np.asarray(rec.electric[0]).tobytes()
        e.close()
    assert first[None] == first["host"] and len({first["host"], first["quiet"], first["random"]}) == 3
    for word in ("quietly", "hostX", "randomised_by_more_than_sixteen_characters", "Quiet", ""):
        r = subprocess.run([exe], cwd=str(tmp_path), env=dict(base, PIC1DP_LOAD=word), capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "PIC1DP_LOAD must be host, random or quiet" in r.stdout + r.stderr, word
