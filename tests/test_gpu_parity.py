"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on
identical seeded inputs.  Bar: bit-exact for positions, velocities, cell
indices, counts and (given identical charge) the field solve; weights within a
few ulp (exp: OCML vs libm); charge/energy within 1e-12 / 1e-10 relative
(summation order; BASELINE.json north_star tolerance 1e-10).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import DIST_CASES
from util import both_inputs, relerr, ulp_diff

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
N_SMALL = 200003          # odd on purpose: exercises the scalar tail
ENERGY_RTOL = 1e-10       # north_star: field energy and growth rate within 1e-10 relative
CHARGE_RTOL = 1e-12


def pair(oracle, amd, npe=1, load=True, **kw):
    kw.setdefault("nparticle_max", N_SMALL)
    kw.setdefault("nx", 64)
    o, g = both_inputs(oracle, amd, **kw)
    sim = oracle.Sim(o, npe=npe)
    eng = amd.Pic1dp(g, npe=npe)
    if load:
        assert sim.load() == 0
        eng.particle_load()
    return sim, eng


def smooth_field(nx, seed=0, amp=0.05):
    rng = np.random.default_rng(seed)
    ix = np.arange(nx)
    return amp * np.sin(2 * np.pi * ix / nx + 0.3) + 0.2 * amp * rng.standard_normal(nx)


# largest distance (ulp) between the device's exp and libm's on the weight equation's
# argument range that the w tolerance below is derived from; test_device_exp_against_libm
# measures it and fails if it is exceeded
EXP_ULP_MAX = 2


def w_cancellation(inp, v):
    """kappa = (|a| + |b|) / |a + b| of the numerator of -f0'/f0 at v
    (src/pic1dp_interaction.F90:278-321): a rounding difference of the two exp() enters
    tmp2 -- and the weight update -- amplified by it.  1 where no exp is involved."""
    T, T2, m = inp.species_temperature[0], inp.species_temperature2[0], inp.species_mass[0]
    den, v0 = inp.species_density[0], inp.species_v0[0]
    if inp.iptcldist == 2:
        a = (v + v0) * np.exp(-(v + v0) ** 2 / (2.0 * T / m))
        b = (v - v0) * np.exp(-(v - v0) ** 2 / (2.0 * T / m))
    elif inp.iptcldist == 3:
        a = den * v / (T / m) * np.exp(-v ** 2 / (2.0 * T / m)) / np.sqrt(T / m)
        b = (1.0 - den) * (v - v0) / (T2 / m) * np.exp(-(v - v0) ** 2 / (2.0 * T2 / m)) / np.sqrt(T2 / m)
    else:
        return np.ones_like(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = (np.abs(a) + np.abs(b)) / np.abs(a + b)
    return np.where(np.isfinite(k), k, 1e300)


def dlnf0_pieces(inp, v):
    """-f0'/f0 of the two-Maxwellian distributions in extended precision, in the pieces the error bounds below
    are made of (src/pic1dp_interaction.F90:278-321; pic1dp_amd/csrc/device_math.hpp dlnf0_one_exp): with rho the
    ratio of the two Maxwellians and L = ln rho, tmp2 = (A + rho B)/(1 + rho) = M + D tanh(L/2).
    Returns dict(tmp2, M, D, L, argmag = the magnitude of the two exp arguments the reference form rounds,
    Lmag = the magnitude of the terms the one-exp form's L is summed from)."""
    ld = np.longdouble
    v = np.asarray(v, dtype=ld)
    T, T2, m = ld(inp.species_temperature[0]), ld(inp.species_temperature2[0]), ld(inp.species_mass[0])
    den, v0 = ld(inp.species_density[0]), ld(inp.species_v0[0])
    tm, tm2 = T / m, T2 / m
    if inp.iptcldist == 3:
        A, B = v / tm, (v - v0) / tm2
        with np.errstate(divide="ignore"):
            lnK = np.log((1 - den) * np.sqrt(tm)) - np.log(den * np.sqrt(tm2))     # -inf without a beam
        a1, a2 = v * v / (2 * tm), (v - v0) ** 2 / (2 * tm2)
        L = lnK + a1 - a2
        h1, h2 = 1 / (2 * tm), 1 / (2 * tm2)
        Lmag = np.abs(h1 - h2) * v * v + np.abs(2 * h2 * v0 * v) + np.abs(lnK - h2 * v0 * v0)
    elif inp.iptcldist == 2:
        A, B = (v - v0) / tm, (v + v0) / tm
        a1, a2 = (v + v0) ** 2 / (2 * tm), (v - v0) ** 2 / (2 * tm)
        L = -2 * v * v0 / tm
        Lmag = np.abs(L)
    else:
        raise ValueError("no exp in this distribution")
    M, D = (A + B) / 2, (B - A) / 2
    return dict(tmp2=M + D * np.tanh(L / 2), M=M, D=D, L=L, argmag=a1 + a2, argmax=np.maximum(a1, a2), Lmag=Lmag)


def dlnf0_bound(pc, one_exp):
    """how far an evaluation of -f0'/f0 may lie from the exact value (absolute).  The ratio rho of the two
    Maxwellians carries the rounding of the exp arguments -- relative 2^-53 each, i.e. ABSOLUTE |argument| 2^-53
    in the exponent -- plus the exp itself (EXP_ULP_MAX) and a few operations; it enters tmp2 with the
    sensitivity D 2 rho/(1 + rho)^2 <= D/2; M and D t then round at the scale |M| + |D| (where they cancel --
    the minimum of f0 between the two humps -- that is the kappa of the reference's numerator)."""
    f = np.float64
    E = np.exp(-np.abs(pc["L"]))
    sens = 2 * E / (1 + E) ** 2
    mag = 3 * pc["Lmag"] if one_exp else 2 * pc["argmag"]
    drho = EPS * (mag + 2 * (EXP_ULP_MAX + 1) + 8)
    with np.errstate(invalid="ignore"):
        ratio_term = np.where(sens > 0, np.abs(pc["D"]) * sens * drho, 0)     # one Maxwellian absent: rho = 0 or inf
    return (ratio_term + 8 * EPS * (np.abs(pc["M"]) + np.abs(pc["D"]))).astype(f)


def assert_w_close_one_exp(inp, v, w_gpu, w_orc, wb_orc):
    """w = wb + dt tmp1 tmp2 Z/m (:329) with tmp2 from the one-exp form on the device and from the reference's
    operation order in the CPU arithmetic: both lie within their bound of the exact value (dlnf0_bound), the
    update is tmp2 times dt tmp1 Z/m = upd / tmp2, three products and a division add 3 ulp of the update, the
    final sum half an ulp of w"""
    pc = dlnf0_pieces(inp, v)
    upd = np.abs(w_orc - wb_orc)
    tmp2 = np.abs(pc["tmp2"]).astype(np.float64)
    d = dlnf0_bound(pc, True) + dlnf0_bound(pc, False)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(tmp2 > 4 * d, upd / (tmp2 - d), np.inf)   # |dt tmp1 Z/m|, from the oracle's own update
    tol = 2.0 * (scale * d + 3 * EPS * upd + 0.5 * EPS * np.abs(w_orc)) + 1e-300
    # where tmp2 itself is within a few bounds of zero the update is rounding: bound by the weights' scale
    tol = np.where(np.isfinite(tol), tol, 64 * EPS * (np.abs(w_orc) + np.abs(wb_orc)))
    err = np.abs(w_gpu - w_orc)
    bad = err > tol
    assert not bad.any(), "w off by %g (tolerance %g, update %g, tmp2 %g) at %d of %d" % (
        err[bad].max(), tol[bad][np.argmax(err[bad])], upd[bad][np.argmax(err[bad])], tmp2[bad][np.argmax(err[bad])],
        np.flatnonzero(bad)[0], bad.sum())


def one_exp_active(probe, inp):
    """does the library evaluate -f0'/f0 of this input's species in the one-exp form (default for iptcldist 2, 3;
    PIC1DP_DLNF0=ref: the reference's operation order)"""
    return inp.deltaf == 1 and probe.species_const(probe.species(inp))["one_exp"] == 1


def assert_w_close(w_gpu, w_orc, wb_orc, exact, kappa=None):
    """w = wb + dt*tmp1*tmp2*Z/m (:329).  Everything but exp() is the same IEEE
    operation on both sides; with exp within EXP_ULP_MAX ulp of libm each of the four
    exp-bearing terms of tmp2 is within EXP_ULP_MAX + 1 ulp, the quotient within
    (EXP_ULP_MAX + 1) * (kappa + 1) + 1, the update after its three products and one
    division by m within that + 2, and the final sum adds half an ulp of w: allow twice that."""
    if exact:
        assert np.array_equal(w_gpu, w_orc)
        return
    upd = np.abs(w_orc - wb_orc)
    kap = np.ones_like(upd) if kappa is None else kappa
    err = np.abs(w_gpu - w_orc)
    tol = 2.0 * (((EXP_ULP_MAX + 1) * (kap + 1.0) + 3.0) * EPS * upd + 0.5 * EPS * np.abs(w_orc)) + 1e-300
    # kappa -> infinity means a + b -> 0 and an update near zero: bound by the update scale itself there
    tol = np.where(kap >= 1e299, 64 * EPS * (np.abs(w_orc) + np.abs(wb_orc)), tol)
    bad = err > tol
    assert not bad.any(), "w off by %g (tolerance %g, update %g, kappa %g) at %d" % (
        err[bad].max(), tol[bad][np.argmax(err[bad])], upd[bad][np.argmax(err[bad])], kap[bad][np.argmax(err[bad])],
        np.flatnonzero(bad)[0])


def test_device_exp_against_libm(oracle_mod, probe):
    """the one operation of the push that is not bit-identical by construction: the
    device's exp (OCML) against libm's on the arguments the weight equation forms,
    -(v -+ v0)^2 / (2T/m) with |v| <= v_max + drift: [-260, 0], dense near 0, plus the
    rest of the double range that does not overflow"""
    import ctypes as C
    rng = np.random.default_rng(7)
    x = np.concatenate([-260.0 * rng.random(3_000_000), -rng.random(1_000_000) ** 4, -745.0 * rng.random(500_000),
                        700.0 * rng.random(500_000), -np.logspace(-300, 2, 20001), [0.0, -0.0]])
    y = probe.device_exp(x)
    ref = np.empty_like(x)
    oracle_mod.lib().orc_exp_array(x, ref, x.size)
    d = ulp_diff(y, ref)
    assert d.max() <= EXP_ULP_MAX, "device exp differs from libm by %d ulp at x = %r" % (d.max(), x[np.argmax(d)])
    # and it is not the same function: a silent switch to a bit-identical exp would make the
    # exp-bearing w comparisons exact -- worth knowing, not an error
    print("device exp vs libm: max %d ulp, %.3f %% of arguments differ" % (d.max(), 100.0 * np.mean(d > 0)))


EXP_DIST_CASES = [(n, k) for n, k in DIST_CASES if k.get("iptcldist", 3) in (2, 3)] + [
    ("bump_hot_beam", dict(iptcldist=3, species_temperature=[0.5], species_temperature2=[4.0], species_density=[0.6],
                           species_v0=[3.0])),
    ("bump_heavy", dict(iptcldist=3, species_temperature=[0.013], species_temperature2=[0.02],
                        species_mass=[1836.15267343], species_density=[0.9], species_v0=[0.01])),
    ("bump_no_beam", dict(iptcldist=3, species_density=[1.0])),
]


@pytest.mark.parametrize("name,kw", EXP_DIST_CASES, ids=lambda v: v if isinstance(v, str) else "")
def test_dlnf0_forms_against_extended_precision(amd, probe, name, kw):
    """-f0'/f0 (src/pic1dp_interaction.F90:278-321) as the marker kernels evaluate it, on its own: the one-exp
    form (default) and the reference's operation order, each against an 80-bit evaluation, within the bound the
    w tolerances of the push tests are built from (dlnf0_bound) -- over the loaded velocity range, beyond it
    (a marker the instability has accelerated), at the humps, at the minimum between them (where the
    numerator cancels) and at 0"""
    inp = amd.make_input(nparticle_max=16, **kw)
    sp = probe.species(inp)
    assert probe.species_const(sp)["one_exp"] == 1
    rng = np.random.default_rng(5)
    v0 = inp.species_v0[0]
    v = np.concatenate([rng.uniform(-8, 8, 2_000_000), rng.uniform(-40, 40, 500_000), rng.normal(v0, 0.01, 100_000),
                        rng.normal(0.0, 1e-3, 100_000), np.linspace(-8, 8, 100_001), [0.0, -0.0, v0, -v0, 1e-300, 200.0]])
    pc = dlnf0_pieces(inp, v)
    exact = pc["tmp2"]
    for form in (1, 0):
        got = probe.dlnf0(sp, v, form)
        err = np.abs(got.astype(np.longdouble) - exact).astype(np.float64)
        bound = dlnf0_bound(pc, form == 1)
        vv = v
        if form == 0:
            # the reference's operation order loses its ratio where a Maxwellian leaves the normal range (exp
            # arguments beyond ~ -700: denormal, then 0/0) -- far outside the loaded |v| <= 8; the one-exp form has
            # no such limit.  Compared where both are normal numbers.
            ok = np.asarray(pc["argmax"] < 690.0)
            assert ok.sum() > 1000 and np.isfinite(got[ok]).all()
            if name == "bump_on_tail":
                assert ok[np.abs(v) <= 12].all()
            err, bound, vv = err[ok], bound[ok], v[ok]
        else:
            assert np.isfinite(got).all()
        worst = np.argmax(err / bound)
        assert (err <= bound).all(), "form %d: off by %g (bound %g) at v = %r" % (form, err[worst], bound[worst], vv[worst])
        print("%s form %d: max error / bound %.3f, max error %.3g" % (name, form, (err / bound).max(), err.max()))


# --------------------------------------------------------------------------
# initial condition
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", DIST_CASES + [("gaussian_markers", dict(iptcldist=0, imarker=1))],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_particle_load_bit_exact(oracle_mod, amd, name, kw):
    sim, eng = pair(oracle_mod, amd, **kw)
    got = eng.particles_download()
    for k in "xvpw":
        assert np.array_equal(got[k], sim.gather(k)), k


def test_particle_load_virtual_ranks(oracle_mod, amd):
    sim, eng = pair(oracle_mod, amd, npe=4)
    assert eng.local_sizes() == (N_SMALL, N_SMALL)
    got = eng.particles_download()
    for k in "xvpw":
        assert np.array_equal(got[k], sim.gather(k)), k


def test_unloaded_tail_slots(oracle_mod, amd):
    """species_nparticle_init < nparticle_max: particle_np < local size
    (src/pic1dp_particle.F90:240-248)"""
    sim, eng = pair(oracle_mod, amd, npe=2, nparticle_max=100001, species_nparticle_init=[90000])
    nalloc, npv = eng.local_sizes()
    assert nalloc == 100001 and npv == 90000
    assert sim.rank_np(0) + sim.rank_np(1) == 90000
    got = eng.particles_download()
    assert np.array_equal(got["x"][:npv], sim.gather("x"))
    # energy sums run over the whole vector, tails included
    es = eng.energy_sums()
    assert relerr(es, sim.energy_sums()) < 1e-12
    eng.interaction_collect_charge()
    sim.collect_charge()
    assert relerr(eng.get_field()["chargeden"], sim.get_field()[1]) < CHARGE_RTOL


# --------------------------------------------------------------------------
# deposit
# --------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [2, 64, 192, 1024, 4096, 8192])
def test_collect_charge(oracle_mod, amd, nx):
    sim, eng = pair(oracle_mod, amd, nx=nx)
    # push x out of [0, lx) first so the wrap does real work
    E = smooth_field(nx)
    sim.set_field(E)
    eng.set_electric(E)
    sim.push(1)
    eng.interaction_push_particle(1)
    sim.collect_charge()
    eng.interaction_collect_charge()
    x_gpu = eng.particles_download()["x"]
    assert np.array_equal(x_gpu, sim.gather("x"))                  # wrapped x, bit-exact
    assert x_gpu.min() >= 0.0 and x_gpu.max() <= sim.inp.lx
    # integer outputs: cell index per marker and per-cell counts
    ix_gpu, cnt_gpu = eng.cell_indices()
    xs = sim.gather("x")
    q = sim.gather("w")
    ix_o = np.empty(xs.size, dtype=np.int32)
    cnt_o = np.zeros(nx, dtype=np.int64)
    oracle_mod.lib().orc_deposit_species_idx(C.byref(sim.inp), xs.size, xs.copy(), q,
                                             np.zeros(nx), ix_o, cnt_o)
    assert np.array_equal(ix_gpu, ix_o)
    assert np.array_equal(cnt_gpu, cnt_o)
    assert cnt_gpu.sum() == xs.size
    assert relerr(eng.get_field()["chargeden"], sim.get_field()[1]) < CHARGE_RTOL


def test_collect_charge_edge_positions(oracle_mod, amd):
    """positions on and beyond the period boundaries, signed zeros, the
    x + lx -> lx rounding case and far-out values (general fmod)"""
    nx = 32
    sim, eng = pair(oracle_mod, amd, load=False, nparticle_max=64, nx=nx)
    lx = sim.inp.lx
    x = np.array([0.0, -0.0, lx, np.nextafter(lx, 0), np.nextafter(lx, 2 * lx), -1e-300, -1e-17,
                  -5e-324, 2.5 * lx, -3.2 * lx, 1e6 * lx + 0.1, -1e6 * lx - 0.1, lx / nx,
                  np.nextafter(lx / nx, 0), 2 * lx, -lx, np.nextafter(-lx, 0), 0.5 * lx] * 4)[:64]
    rng = np.random.default_rng(1)
    v = rng.uniform(-8, 8, 64)
    p = rng.uniform(0.5, 1.5, 64)
    w = rng.uniform(-1, 1, 64)
    for k, a in zip("xvpw", (x, v, p, w)):
        sim.array(0, 0, k)[:] = a
    eng.particles_upload(x, v, p, w)
    sim.collect_charge()
    eng.interaction_collect_charge()
    xg = eng.particles_download()["x"]
    xo = sim.gather("x")
    assert np.array_equal(xg.view(np.int64), xo.view(np.int64))    # incl. the sign of zero
    assert relerr(eng.get_field()["chargeden"], sim.get_field()[1]) < 1e-13


@pytest.mark.parametrize("n", [1, 2, 3, 5, 127, 1025])
def test_tiny_particle_counts(oracle_mod, amd, n):
    sim, eng = pair(oracle_mod, amd, nparticle_max=n, nx=16)
    for _ in range(3):
        sim.step(1)
        eng.step(1)
    g = eng.particles_download()
    assert np.array_equal(g["x"], sim.gather("x"))
    assert np.array_equal(g["v"], sim.gather("v"))
    assert relerr(eng.get_field()["electric"], sim.get_field()[0]) < 1e-10


# --------------------------------------------------------------------------
# field solve
# --------------------------------------------------------------------------
@pytest.mark.parametrize("nx,modes", [(64, [1]), (192, [1]), (192, [1, 2, 5]), (1024, [1]), (4096, [1, 3]),
                                      (77, [1, 2]), (1023, [1]), (9, [1, 3]), (31, [2]),   # odd: unaligned LDS rows
                                      (250, list(range(1, 65))), (250, list(range(1, 126))),
                                      (256, list(range(1, 129))), (1000, list(range(1, 500))),
                                      (2048, list(range(1, 1025)))],
                         ids=lambda v: str(v) if isinstance(v, int) else "m%d" % len(v))
@pytest.mark.parametrize("npe", [1, 2, 4, 7, 8, 16])
def test_field_solve_bit_exact(oracle_mod, amd, nx, modes, npe):
    """same chargeden in -> identical E, mode_re, mode_im: the forward sums run in the reference's order -- one
    rank (SeqAIJ): ascending ix, one thread per mode component; npe ranks (MPI-AIJ, `mpiexec -n 4` is the
    reference's own launch line): every rank's PETSC_DECIDE row block from zero, the blocks added owner first then
    in rank order (oracle: orc_field_solve_ranks), here as partial chains side by side; the inverse takes, row by
    row, the mode entries of the row's own rank first (MPI-AIJ's diagonal block), then the others"""
    if npe > 1 and nx > 1100 and len(modes) > 600:
        pytest.skip("one large many-mode case per order is enough")
    sim, eng = pair(oracle_mod, amd, load=False, npe=npe, nparticle_max=max(16, npe), nx=nx, nmode=len(modes), modes=modes)
    rng = np.random.default_rng(nx)
    rho = rng.standard_normal(nx) * 1e-3
    E, re, im = oracle_mod.Field(sim.inp).solve(rho, npe)
    if npe > 1 and nx >= 64:   # the order is observable: not the one-rank sums
        E1, re1, im1 = oracle_mod.Field(sim.inp).solve(rho, 1)
        assert not (np.array_equal(re, re1) and np.array_equal(im, im1)) or len(modes) == 1
        if len(modes) >= 60:   # so is the inverse's: the plain ascending sum of the same modes gives another E
            fre, fim, _ = oracle_mod.Field(sim.inp).tables()
            asc = 2.0 * np.cumsum(np.concatenate([fre * re, fim * im], axis=1), axis=1)[:, -1]
            assert not np.array_equal(asc, E)
    eng.set_chargeden(rho)
    eng.field_solve_electric()
    f = eng.get_field()
    assert np.array_equal(f["mode_re"], re)
    assert np.array_equal(f["mode_im"], im)
    assert np.array_equal(f["electric"], E)
    assert abs(eng.field_energy() - oracle_mod.lib().orc_field_energy(C.byref(sim.inp), E)) <= 64 * EPS * abs(eng.field_energy())


@pytest.mark.parametrize("chain", ["1", "0"], ids=["matrix_unit_chain", "one_lane_chain"])
@pytest.mark.parametrize("npe", [1, 2])
def test_engine_two_virtual_ranks_nx128_chain_on_and_off(oracle_mod, amd, monkeypatch, npe, chain):
    """The configuration of round 4's mid-round red run (gpurun_out/r4o, profiles/README.md: `field_energy_end = nan` out
    of bench.py's two-rank rehearsal AND out of the one-process engine with two virtual ranks, nx 128, 3e6 markers, while
    the serial sums through the matrix unit were going in) as a direct test of the engine: every field energy of a run
    finite and within 1e-10 of the oracle's npe-rank run, the solve of one charge density bit-identical to the oracle's --
    with the create()-time self-test deciding for the matrix unit and with the one-lane chains insisted on -- and the
    npe-rank order never routed through the matrix unit (its rows are rank blocks, not the one-rank sum)."""
    monkeypatch.setenv("PIC1DP_CHAIN_MFMA", chain)
    sim, eng = pair(oracle_mod, amd, npe=npe, nparticle_max=300_000, nx=128)
    verdict, used = eng.kernel_stats(9)
    assert used == (1 if (chain == "1" and verdict == 1.0) else 0)
    t, eo, eg = run_both(sim, eng, 40)
    assert np.all(np.isfinite(eg)) and np.all(eg > 0.0)
    assert np.max(np.abs(eg / eo - 1.0)) < ENERGY_RTOL
    rho = np.random.default_rng(128).standard_normal(128) * 1e-3
    E, re, im = oracle_mod.Field(sim.inp).solve(rho, npe)
    eng.set_chargeden(rho)
    eng.field_solve_electric()
    f = eng.get_field()
    assert np.array_equal(f["mode_re"], re) and np.array_equal(f["mode_im"], im) and np.array_equal(f["electric"], E)


def test_field_solve_full_spectrum(oracle_mod, amd):
    """every mode 1..nx/2-1 kept (the many-mode kernels).  The solve is
    then the spectral integral of a zero-mean chargeden without its Nyquist part:
    dE/dx = rho in the spectral sense, checked with numpy's FFT; and a whole run
    with 300 kept modes follows the oracle like the one-mode runs do."""
    nx = 512
    modes = list(range(1, nx // 2))
    eng = amd.Pic1dp(amd.make_input(nparticle_max=16, nx=nx, nmode=len(modes), modes=modes))
    rng = np.random.default_rng(7)
    rho = rng.standard_normal(nx)
    rho -= rho.mean()
    eng.set_chargeden(rho)
    eng.field_solve_electric()
    E = eng.get_field()["electric"]
    k = 2 * np.pi / eng.inp.lx * np.fft.fftfreq(nx, 1.0 / nx)
    rk = np.fft.fft(rho)
    rk[nx // 2] = 0.0
    ek = np.zeros(nx, dtype=complex)
    ek[1:] = rk[1:] / (1j * k[1:])
    want = np.fft.ifft(ek).real
    assert np.max(np.abs(E - want)) < 1e-12 * np.max(np.abs(want))
    sim, eng = pair(oracle_mod, amd, nparticle_max=20000, nx=640, nmode=300, modes=list(range(1, 301)))
    t, eo, eg = run_both(sim, eng, 5)
    assert np.max(np.abs(eg / eo - 1.0)) < ENERGY_RTOL


def test_field_solve_analytic(amd):
    """the reference's field_test (src/pic1dp_field.F90:276-309): rho = cos(2 pi ix/nx)
    with mode 1 kept gives E = lx/(2 pi) sin(2 pi ix/nx)"""
    nx = 192
    eng = amd.Pic1dp(amd.make_input(nparticle_max=16, nx=nx))
    ix = np.arange(nx)
    eng.set_chargeden(np.cos(2 * np.pi * ix / nx))
    eng.field_solve_electric()
    E = eng.get_field()["electric"]
    want = eng.inp.lx / (2 * np.pi) * np.sin(2 * np.pi * ix / nx)
    assert np.max(np.abs(E - want)) < 1e-13 * eng.inp.lx


# --------------------------------------------------------------------------
# push
# --------------------------------------------------------------------------
PUSH_CASES = [(n, kw, lin) for n, kw in DIST_CASES for lin in (0, 1)]


@pytest.mark.parametrize("name,kw,linear", PUSH_CASES, ids=lambda v: str(v) if not isinstance(v, dict) else "")
@pytest.mark.parametrize("form", ["one_exp", "ref"])
def test_push_particle(oracle_mod, amd, probe, monkeypatch, name, kw, linear, form):
    """interaction_push_particle against the oracle on identical particles and
    field: x and v bit-exact; w bit-exact where no exp is involved, else within
    the bound derived from the exp's measured distance to libm and the conditioning of
    -f0'/f0 -- with the one-exp form of -f0'/f0 (the default) and with the reference's
    operation order (PIC1DP_DLNF0=ref)"""
    if form == "ref":
        if kw.get("iptcldist", 3) not in (2, 3):
            pytest.skip("no exp in this distribution: one form only")
        monkeypatch.setenv("PIC1DP_DLNF0", "ref")
    sim, eng = pair(oracle_mod, amd, linear=linear, **kw)
    nx = sim.inp.nx
    exact_w = sim.inp.iptcldist in (0, 1)
    one_exp = one_exp_active(probe, sim.inp)
    assert one_exp == (form == "one_exp" and not exact_w)
    for irk, seed in ((1, 11), (2, 12)):
        E = smooth_field(nx, seed)
        sim.set_field(E)
        eng.set_electric(E)
        wb = sim.gather("w") if irk == 1 else sim.gather("wb")
        v_at = sim.gather("v")                                 # v the derivatives are evaluated at
        kappa = w_cancellation(sim.inp, v_at)
        sim.push(irk)
        eng.interaction_push_particle(irk)
        g = eng.particles_download()
        assert np.array_equal(g["x"], sim.gather("x")), "x irk=%d" % irk
        assert np.array_equal(g["v"], sim.gather("v")), "v irk=%d" % irk
        if one_exp:
            assert_w_close_one_exp(sim.inp, v_at, g["w"], sim.gather("w"), wb)
        else:
            assert_w_close(g["w"], sim.gather("w"), wb, exact_w, kappa)
        if irk == 1:
            b = eng.particles_download_bak()
            assert np.array_equal(b["xb"], sim.gather("xb"))
            assert np.array_equal(b["vb"], sim.gather("vb"))
            assert np.array_equal(b["wb"], sim.gather("wb"))
            # keep both sides on the same weights for the second sub-step
            eng_w = g["w"]
            sim_w = sim.gather("w")
            if not np.array_equal(eng_w, sim_w):
                sim.array(0, 0, "w")[:] = eng_w
        sim.collect_charge()
        eng.interaction_collect_charge()


def test_push_full_f(oracle_mod, amd):
    sim, eng = pair(oracle_mod, amd, deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0])
    for it in range(3):
        for irk in (1, 2):
            sim.push(irk)
            eng.interaction_push_particle(irk)
            sim.collect_charge()
            eng.interaction_collect_charge()
            sim.solve_field()
            eng.field_solve_electric()
            # the field differs by summation order only; keep both sides on one field
            sim.set_field(eng.get_field()["electric"])
    g = eng.particles_download()
    assert np.array_equal(g["x"], sim.gather("x"))
    assert np.array_equal(g["v"], sim.gather("v"))
    assert np.array_equal(g["w"], sim.gather("w"))   # w is not evolved in full-f
    assert relerr(eng.get_field()["chargeden"], sim.get_field()[1]) < 1e-9  # O(1) density minus n0


# --------------------------------------------------------------------------
# fused sub-step and whole runs
# --------------------------------------------------------------------------
def test_fused_substep_equals_separate_calls(amd):
    inp = amd.make_input(nparticle_max=N_SMALL, nx=128)
    a, b = amd.Pic1dp(inp), amd.Pic1dp(inp)
    for e in (a, b):
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()
    b.set_electric(a.get_field()["electric"])   # atomics order: E may differ in the last bit
    for it in range(4):
        for irk in (1, 2):
            a.substep(irk)
            b.interaction_push_particle(irk)
            b.interaction_collect_charge()
            b.field_solve_electric()
            # charge sums differ in order only; resynchronise the field so that
            # the particle comparison stays bit-exact
            assert relerr(a.get_field()["electric"], b.get_field()["electric"]) < 1e-11
            b.set_electric(a.get_field()["electric"])
    ga, gb = a.particles_download(), b.particles_download()
    for k in "xvw":
        assert np.array_equal(ga[k], gb[k]), k


STEP_CASES = [(n, kw, lin) for n, kw in DIST_CASES for lin in (0, 1)] + [
    ("full_f", dict(deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0]), 0)]


@pytest.mark.parametrize("stream", ["plain", "nt"])
@pytest.mark.parametrize("name,kw,linear", STEP_CASES, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_whole_step_recompute_equals_substeps(amd, probe, monkeypatch, name, kw, linear, stream):
    """pic1dp_hip_step's default path never stores the half-step state: the
    second kernel recomputes it from the step-start state and field.  Given the
    same two fields it must reproduce the two-sub-step path bit for bit -- in
    both instantiations of the kernels: plain accesses for cache-resident marker
    counts, non-temporal ones once the marker state exceeds the whole-step
    kernels' threshold of 288 MiB (settings.hpp nt_threshold_full; 9 437 185
    markers here, the smallest count with 32 n beyond it and an odd one: the
    product build has no knob for the threshold; a tuning build's
    PIC1DP_NT_THRESHOLD_MB reaches them at the small count).  On a product
    build the sub-step kernels of b stay plain at either count
    (nt_threshold_half: 2 GiB)."""
    n = N_SMALL
    if stream == "nt":
        if amd.tuning_build():
            monkeypatch.setenv("PIC1DP_NT_THRESHOLD_MB", "0")
        else:
            n = 9_437_185
    # the launch of the whole-step kernels is non-temporal exactly when the state exceeds the threshold (capi_step.cpp plan_step)
    threshold = probe.host_settings()["nt_threshold_full"]
    assert (32.0 * n > threshold) == (stream == "nt"), (n, threshold)
    print("%s: %d B of state against nt_threshold_full = %d B: a %s launch" % (
        stream, 32 * n, threshold, "non-temporal" if 32.0 * n > threshold else "plain"))
    inp = amd.make_input(nparticle_max=n, nx=96, linear=linear, **kw)
    a, b = amd.Pic1dp(inp), amd.Pic1dp(inp)
    for e in (a, b):
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()
    b.set_electric(a.get_field()["electric"])
    for it in range(3 if n == N_SMALL else 1):
        a.step(1)                                   # whole-step kernels
        b.substep(1)                                # materialised half-step state
        assert relerr(b.get_field()["electric"], a.get_field_half()) < 1e-10
        b.set_electric(a.get_field_half())
        b.substep(2)
        assert relerr(b.get_field()["electric"], a.get_field()["electric"]) < 1e-10
        b.set_electric(a.get_field()["electric"])
        ga, gb = a.particles_download(), b.particles_download()
        for k in "xvw":
            assert np.array_equal(ga[k], gb[k]), (k, it)
    # and the explicit two-sub-step mode of step() is the same thing as substep()
    c = amd.Pic1dp(inp)
    c.particle_load()
    c.interaction_collect_charge()
    c.field_solve_electric()
    c.set_step_mode(1)
    c.step(1)
    assert relerr(c.get_field()["electric"], a.get_field()["electric"]) < 1.0  # ran
    assert c.itime == 1


def test_whole_step_falls_back_for_large_grids(oracle_mod, amd):
    """nx = 8192 needs 196 KB for three grid tiles: step() uses the ping-pong
    sub-steps instead and still matches the oracle"""
    sim, eng = pair(oracle_mod, amd, nparticle_max=50000, nx=8192)
    t, eo, eg = run_both(sim, eng, 10)
    assert np.max(np.abs(eg / eo - 1.0)) < ENERGY_RTOL
    sim, eng = pair(oracle_mod, amd, nparticle_max=50000, nx=4096)      # 3 tiles fit: recompute path
    t, eo, eg = run_both(sim, eng, 10)
    assert np.max(np.abs(eg / eo - 1.0)) < ENERGY_RTOL


def test_step_modes_agree_with_oracle(oracle_mod, amd):
    for mode in (0, 1):
        sim, eng = pair(oracle_mod, amd, nparticle_max=100000, nx=64)
        eng.set_step_mode(mode)
        t, eo, eg = run_both(sim, eng, 60)
        assert np.max(np.abs(eg / eo - 1.0)) < ENERGY_RTOL, mode
        g = eng.particles_download()
        assert np.max(np.abs(g["x"] - sim.gather("x"))) < 1e-9


def run_both(sim, eng, nsteps):
    sim.collect_charge()
    sim.solve_field()
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    e_o = [sim.field_energy()]
    e_g0 = eng.field_energy()
    for _ in range(nsteps):
        sim.step(1)
        e_o.append(sim.field_energy())
    eng.energy_history_reset()
    eng.step(nsteps)
    e_g = np.concatenate([[e_g0], eng.energy_history()])
    t = np.arange(nsteps + 1) * sim.inp.dt
    return t, np.array(e_o), e_g


def test_run_field_energy_and_growth_rate(oracle_mod, amd):
    """short run inside the linear phase: int E^2 dx at every step and the fitted
    growth rate (tools/OutputData.py:153-170) within 1e-10 relative"""
    sim, eng = pair(oracle_mod, amd, nparticle_max=200000, nx=64)
    t, eo, eg = run_both(sim, eng, 300)
    assert eg.size == eo.size
    assert np.max(np.abs(eg / eo - 1.0)) < ENERGY_RTOL
    g_o = oracle_mod.growthrate_energy_fit(t, eo, 5.0, 15.0)
    g_g = oracle_mod.growthrate_energy_fit(t, eg, 5.0, 15.0)
    assert abs(g_g / g_o - 1.0) < ENERGY_RTOL
    assert eng.itime == 300 and abs(eng.time - sim.time) == 0.0
    assert relerr(eng.energy_sums(), sim.energy_sums()) < 1e-11


@pytest.mark.parametrize("name,kw", [
    ("two_stream2", dict(iptcldist=2, species_density=[1.0], species_v0=[3.0])),
    ("landau", dict(iptcldist=0, species_density=[1.0], species_v0=[0.0], lx=4 * np.pi, linear=1)),
    ("two_stream1", dict(iptcldist=1, species_density=[1.0])),
    ("three_modes", dict(nmode=3, modes=[1, 2, 3], init_nmode=2, init_mode=[1, 2],
                         init_mode_cos=[2e-6, 0.0], init_mode_sin=[1e-5, 3e-6])),
], ids=lambda v: v if isinstance(v, str) else "")
def test_run_other_configs(oracle_mod, amd, name, kw):
    sim, eng = pair(oracle_mod, amd, nparticle_max=100000, nx=48, **kw)
    t, eo, eg = run_both(sim, eng, 100)
    assert np.max(np.abs(eg / eo - 1.0)) < ENERGY_RTOL


def test_run_virtual_ranks(oracle_mod, amd):
    """one GPU reproducing a 4-rank reference run (4 RNG streams, 4 blocks)"""
    sim, eng = pair(oracle_mod, amd, npe=4, nparticle_max=100002, nx=64)
    t, eo, eg = run_both(sim, eng, 100)
    assert np.max(np.abs(eg / eo - 1.0)) < ENERGY_RTOL


def test_run_two_species(oracle_mod, amd):
    kw = dict(nspecies=2, iptcldist=0, species_charge=[-1.0, 1.0], species_mass=[1.0, 25.0],
              species_temperature=[1.0, 0.5], species_temperature2=[1.0, 1.0],
              species_density=[1.0, 1.0], species_v0=[0.0, 0.0], lx=4 * np.pi)
    sim, eng = pair(oracle_mod, amd, nparticle_max=60000, nx=32, **kw)
    t, eo, eg = run_both(sim, eng, 60)
    assert np.max(np.abs(eg / eo - 1.0)) < ENERGY_RTOL
    for isp in (0, 1):
        g = eng.particles_download(isp)
        assert np.max(ulp_diff(g["x"], sim.gather("x", isp))) <= 2 ** 20  # trajectories follow the 1e-10 field


def test_reference_driver_loop(oracle_mod, amd):
    """Pic1dp.run reproduces the sequencing of src/pic1dp.F90:67-109: output at
    step 0, every output_interval, and at termination"""
    o, g = both_inputs(oracle_mod, amd, nparticle_max=20000, nx=32, time_max=1.2, output_interval=0.5)
    eng = amd.Pic1dp(g)
    eng.particle_load()
    outs = []
    steps = eng.run(on_output=lambda e: outs.append((e.itime, e.field_energy())))
    assert steps == 24                       # 1.2 / 0.05
    assert [i for i, _ in outs] == [0, 10, 20, 24]
    sim = oracle_mod.Sim(o)
    sim.load()
    sim.collect_charge()
    sim.solve_field()
    sim.step(24)
    assert abs(outs[-1][1] / sim.field_energy() - 1.0) < ENERGY_RTOL
    # unfused call sequence gives the same run
    eng2 = amd.Pic1dp(g)
    eng2.particle_load()
    assert eng2.run(fused=False) == 24
    assert abs(eng2.field_energy() / sim.field_energy() - 1.0) < ENERGY_RTOL


# --------------------------------------------------------------------------
# split-phase deposit, diagnostics, errors
# --------------------------------------------------------------------------
def test_split_phase_charge(amd):
    inp = amd.make_input(nparticle_max=50000, nx=64)
    a, b = amd.Pic1dp(inp), amd.Pic1dp(inp)
    a.particle_load()
    b.particle_load()
    a.interaction_collect_charge()
    c2 = b.charge_local()
    with pytest.raises(amd.Pic1dpError):
        b.interaction_push_particle(1)       # waiting for the reduced charge
    b.charge_reduced(c2)
    assert relerr(b.get_field()["chargeden"], a.get_field()["chargeden"]) < CHARGE_RTOL
    assert np.array_equal(a.particles_download()["x"], b.particles_download()["x"])


def test_split_phase_charge_time_loop(amd):
    """a host that keeps its own MPI_Allreduce: push / charge_local / [reduce] /
    charge_reduced / solve_field for whole steps gives the markers of the
    collect_charge loop (both served by the whole-step kernels)"""
    inp = amd.make_input(nparticle_max=N_SMALL, nx=64)
    a, b = amd.Pic1dp(inp), amd.Pic1dp(inp)
    for e in (a, b):
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()
    b.set_electric(a.get_field()["electric"])
    b.kernel_stats_enable(True)
    for it in range(3):
        for irk in (1, 2):
            a.interaction_push_particle(irk)
            a.interaction_collect_charge()
            a.field_solve_electric()
            b.interaction_push_particle(irk)
            b.charge_reduced(b.charge_local())
            b.field_solve_electric()
            assert relerr(b.get_field()["electric"], a.get_field()["electric"]) < 1e-10
            b.set_electric(a.get_field()["electric"])
    ga, gb = a.particles_download(), b.particles_download()
    for k in "xvw":
        assert np.array_equal(ga[k], gb[k]), k
    # whole-step kernels served the noted pushes: three second-sub-step kernels (k_step_full or,
    # with the prediction of the next first sub-step, k_step_one), no separate push kernel
    assert b.kernel_stats(1)[1] == 0 and b.kernel_stats(4)[1] + b.kernel_stats(6)[1] == 3


@pytest.mark.parametrize("kind,nx,modes", [(1, 64, None), (2, 64, None), (1, 2048, None), (2, 4096, None), (1, 64, [1, 2]),
                                           (1, 63, [1, 2])],
                         ids=["tiles", "sums", "tiles-nx2048", "sums-nx4096", "tiles-two-modes", "tiles-two-modes-nx63"])
def test_rccl_allreduce_path_single_rank(oracle_mod, amd, monkeypatch, kind, nx, modes):
    """a 1-rank RCCL communicator: exercises the run-time RCCL binding, the
    unique-id hand-off and the split kernels (charge_local -> ncclAllReduce on
    the engine's stream -> field solve; in a one-pass step: pack -> ONE
    ncclAllReduce -> the paired solve, with the prediction as tiles or as six
    sums) that N > 1 uses; two kept modes: the generic paired solve from the pack (k_field_solve_pair<2>)"""
    monkeypatch.setenv("PIC1DP_PRED_KIND", str(kind))
    kw = dict(nmode=len(modes), modes=modes) if modes else {}
    sim, eng = pair(oracle_mod, amd, nparticle_max=100000, nx=nx, **kw)
    assert eng.predict_kind() == kind
    uid = eng.comm_unique_id()
    assert len(uid) == 128 and any(uid)
    eng.comm_init(uid)
    with pytest.raises(amd.Pic1dpError):
        eng.comm_init(uid)                   # only once
    t, eo, eg = run_both(sim, eng, 40)
    assert np.max(np.abs(eg / eo - 1.0)) < ENERGY_RTOL
    eng.interaction_collect_charge()
    sim.collect_charge()
    assert relerr(eng.get_field()["chargeden"], sim.get_field()[1]) < CHARGE_RTOL
    # and the reference's call sites over the same communicator
    for _ in range(3):
        for irk in (1, 2):
            eng.interaction_push_particle(irk)
            eng.interaction_collect_charge()
            eng.field_solve_electric()
        sim.step(1)
    assert abs(eng.field_energy() / sim.field_energy() - 1.0) < ENERGY_RTOL


@pytest.mark.parametrize("kw", [dict(), dict(nspecies=2, species_charge=[-1.0, 1.0], species_mass=[1.0, 4.0],
                                             species_temperature=[1.0, 1.0], species_temperature2=[1.0, 1.0],
                                             species_density=[0.9, 0.9], species_v0=[5.0, 5.0])],
                         ids=["one_species", "two_species"])
def test_rccl_pack_in_the_marker_launch_equals_the_pack_launch(amd, monkeypatch, kw):
    """on the RCCL path the packing of this rank's charge2 and six sums for the ONE all-reduce of
    a one-pass step (src/pic1dp_interaction.F90:126-135) is done by the last workgroup of the marker launch to finish
    (kernels.hpp StepTail) instead of a launch of its own (PIC1DP_TAIL=0).  Same accumulators, the same additions in
    the same order: bit for bit with one wave of markers per block, 1e-11 where the charge atomics' order varies; with
    two species the tail rides in the second species' launch."""
    monkeypatch.setenv("PIC1DP_PRED_KIND", "2")
    ns = kw.get("nspecies", 1)
    for n, exact in ((96, True), (300_001, False)):
        engs = []
        for tail in ("1", "0"):
            monkeypatch.setenv("PIC1DP_TAIL", tail)
            e = amd.Pic1dp(amd.make_input(nparticle_max=n, nx=64, species_nparticle_init=[n] * ns, **kw))
            e.particle_load()
            e.comm_init(e.comm_unique_id())
            e.interaction_collect_charge()
            e.field_solve_electric()
            e.step(30)
            engs.append(e)
        a, b = engs
        assert a.kernel_stats(10)[1] == 30 and b.kernel_stats(10)[1] == 0
        fa, fb = a.get_field(), b.get_field()
        if exact:
            assert np.array_equal(a.energy_history(), b.energy_history())
            for k in ("electric", "chargeden", "mode_re", "mode_im"):
                assert np.array_equal(fa[k], fb[k]), k
            for isp in range(ns):
                ga, gb = a.particles_download(isp), b.particles_download(isp)
                for k in "xvw":
                    assert np.array_equal(ga[k], gb[k]), (isp, k)
        else:
            assert np.max(np.abs(a.energy_history() / b.energy_history() - 1.0)) < 1e-11
            assert relerr(fa["electric"], fb["electric"]) < 1e-11
        # nothing stale in the accumulators or the ticket: the call sites and a further step() go on from here
        for e in engs:
            e.interaction_collect_charge()
        assert relerr(a.get_field()["chargeden"], b.get_field()["chargeden"]) < (1e-15 if exact else 1e-11)
        for e in engs:
            e.step(3)
        assert np.max(np.abs(a.energy_history()[-3:] / b.energy_history()[-3:] - 1.0)) < 1e-11


def test_error_behaviour(amd):
    inp = amd.make_input(nparticle_max=1000, nx=16)
    eng = amd.Pic1dp(inp)
    with pytest.raises(amd.Pic1dpError) as ei:
        eng.interaction_push_particle(1)     # nothing loaded
    assert ei.value.code == 4
    eng.particle_load()
    with pytest.raises(amd.Pic1dpError) as ei:
        eng.interaction_push_particle(3)
    assert ei.value.code == 1
    with pytest.raises(amd.Pic1dpError):
        amd.Pic1dp(amd.make_input(nparticle_max=1000, nx=16, iptclshape=2))
    with pytest.raises(amd.Pic1dpError):
        amd.Pic1dp(amd.make_input(nparticle_max=1000, nx=16, linear=1, deltaf=0))
    with pytest.raises(amd.Pic1dpError):
        amd.Pic1dp(amd.make_input(nparticle_max=1000, nx=16), nranks=2, rank=0, npe=3)
    bad = amd.make_input(nparticle_max=1000, nx=16, multirand_selftest=0)
    e2 = amd.Pic1dp(bad)
    with pytest.raises(amd.Pic1dpError) as ei:
        e2.particle_load()                   # the reference would hang here
    assert ei.value.code == 6


def test_timers_and_kernel_stats(amd):
    eng = amd.Pic1dp(amd.make_input(nparticle_max=400000, nx=64))
    eng.particle_load()
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    eng.timers_enable(True)
    eng.kernel_stats_enable(True)
    eng.step(5)
    (ms3, n3), (ms4, n4), (ms6, n6) = eng.kernel_stats(3), eng.kernel_stats(4), eng.kernel_stats(6)
    # k_step_half once (first step), then one k_step_one per step: the first sub-step's charge is predicted
    assert n3 == 1 and n4 == 0 and n6 == 5 and ms3 > 0.0 and ms6 > 0.0
    eng.set_step_mode(1)
    eng.step(5)
    ms, n = eng.kernel_stats(0)
    assert n == 10 and ms > 0.0
    assert eng.timer_ms(4) > 0.0 and eng.timer_ms(7) > 0.0   # push_particle, field_electric
    eng.timers_reset()
    assert eng.kernel_stats(0) == (0.0, 0)


def test_sampled_timers_estimate_the_exact_ones(amd):
    """pic1dp_hip_timers_enable(n >= 2): only every n-th launch under a timer id is bracketed by events (an event pair
    costs the stream a dependency: 10-28 % of a default-size run), the time reported is scaled by launches seen /
    launches timed -- within the run-to-run spread of the exact timers on a homogeneous run, and the same results"""
    kw = dict(nparticle_max=2000000, nx=192)
    times, energy = {}, {}
    for every in (1, 8):
        eng = amd.Pic1dp(amd.make_input(**kw))
        eng.particle_load()
        eng.interaction_collect_charge()
        eng.field_solve_electric()
        eng.step(20)
        eng.timers_enable(every)
        for _ in range(160):
            for irk in (1, 2):
                eng.interaction_push_particle(irk)
                eng.interaction_collect_charge()
                eng.field_solve_electric()
        times[every] = (eng.timer_ms(4), eng.timer_ms(7))      # push particle, electric field
        energy[every] = eng.field_energy()
        eng.close()
    assert abs(energy[1] / energy[8] - 1.0) < 1e-12   # (the charge atomics' order)
    for a, b in zip(times[1], times[8]):
        assert a > 0.0 and b > 0.0 and 0.6 < b / a < 1.6, times
    with pytest.raises(amd.Pic1dpError):
        amd.Pic1dp(amd.make_input(nparticle_max=1000, nx=16)).timers_enable(-1)


# --------------------------------------------------------------------------
# full-size properties (BASELINE.json configs 2 and 3): no oracle at this size
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n,nx", [(10**7, 256), (10**8, 1024)], ids=["C2_1e7", "C3_1e8"])
def test_full_size_properties(amd, n, nx):
    eng = amd.Pic1dp(amd.make_input(nparticle_max=n, nx=nx))
    eng.particle_load()
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    lx = eng.inp.lx
    ix, cnt = eng.cell_indices()
    assert cnt.sum() == n and ix.min() >= 0 and ix.max() < nx
    assert np.array_equal(np.bincount(ix, minlength=nx), cnt)
    del ix
    # every marker is counted once; uniform loading: each cell within 6 sigma
    mean = n / nx
    assert np.all(np.abs(cnt - mean) < 6 * np.sqrt(mean))
    # charge conservation: sum(chargeden) * lx/nx == Z * sum(w)
    p = eng.particles_download()
    wsum = -1.0 * np.sum(p["w"], dtype=np.longdouble)
    f = eng.get_field()
    tot = np.sum(f["chargeden"], dtype=np.longdouble) * lx / nx
    scale = np.sum(np.abs(p["w"]), dtype=np.longdouble)
    assert abs(tot - wsum) < 1e-12 * scale
    assert p["x"].min() >= 0.0 and p["x"].max() <= lx
    del p
    # initial field energy of the 1e-5 sin perturbation: (a/k)^2 * lx/2
    k = 2 * np.pi / lx
    assert abs(eng.field_energy() / ((1e-5 / k) ** 2 * lx / 2) - 1.0) < 5e-2
    # a time step keeps every marker and the solve returns a pure mode-1 field
    eng.step(2)
    _, cnt2 = eng.cell_indices()
    assert cnt2.sum() == n
    E = eng.get_field()["electric"]
    spec = np.fft.rfft(E)
    assert np.max(np.abs(np.delete(spec, 1))) < 1e-12 * np.abs(spec[1])
    # idempotence: depositing twice from the same state gives the same charge
    eng.interaction_collect_charge()
    c1 = eng.get_field()["chargeden"]
    eng.interaction_collect_charge()
    assert relerr(eng.get_field()["chargeden"], c1) < CHARGE_RTOL


@pytest.mark.parametrize("kw", [dict(nx=1024), dict(nx=4096, lx=4 * np.pi), dict(nx=192, lx=17.0),
                                dict(nx=64, lx=1.0 / 3.0)], ids=lambda d: "nx%d" % d["nx"])
def test_exact_division_by_lx_device(amd, probe, kw):
    """div_lx (reciprocal + two FMA corrections) against the hardware IEEE
    division on 4e8 generated positions, cell boundaries +- ulps included"""
    inp = amd.make_input(nparticle_max=16, **kw)
    assert probe.div_lx_mismatches(inp.lx, inp.nx, 400_000_000, 77) == 0


@pytest.mark.parametrize("kw", [
    dict(species_temperature=[1.3], species_temperature2=[0.7], species_mass=[1.1]),
    dict(species_temperature=[2.0], species_temperature2=[0.5]),
    dict(species_temperature=[0.013], species_temperature2=[37.0], species_mass=[1836.15267343]),
], ids=["T1.3", "T2", "m1836"])
def test_exact_division_by_species_constant_device(amd, probe, kw):
    """div_const on the device against the hardware IEEE division: 1e8 dividends
    for each of the eight divisor constants of the species (m, T, T/m, T2/m, 2T/m, 2T2/m and the two roots,
    formed as the library forms them: pic1dp_amd/csrc/species.cpp)"""
    inp = amd.make_input(nparticle_max=16, **kw)
    m, T, T2 = inp.species_mass[0], inp.species_temperature[0], inp.species_temperature2[0]
    divisors = [m, T, T / m, T2 / m, 2.0 * T / m, 2.0 * T2 / m, np.sqrt(T / m), np.sqrt(T2 / m)]
    for i, d in enumerate(divisors):
        assert probe.div_const_mismatches(float(d), 100_000_000, 99 + i) == 0, d


@pytest.mark.parametrize("fast", ["0", "1"])
def test_non_unit_species_fast_and_hardware_division_agree(oracle_mod, amd, monkeypatch, tuning, fast):
    """a bump-on-tail species with T, T2, m that are not powers of two: x and v
    bit-exact against the oracle's true divisions with div_const on and off
    (PIC1DP_FAST_DIVC, a tuning build's knob: the product takes div_const wherever
    its host check vouches for the divisors), and the two settings give
    bit-identical weights"""
    kw = dict(iptcldist=3, species_temperature=[1.3], species_temperature2=[0.7], species_mass=[1.1],
              species_density=[0.85], species_v0=[4.5])
    monkeypatch.setenv("PIC1DP_DLNF0", "ref")      # the ten constant divisions live in the reference's operation order
    monkeypatch.setenv("PIC1DP_FAST_DIVC", fast)
    sim, eng = pair(oracle_mod, amd, **kw)
    monkeypatch.setenv("PIC1DP_FAST_DIVC", "0")
    ref = amd.Pic1dp(eng.inp)
    ref.particle_load()
    nx = sim.inp.nx
    for irk, seed in ((1, 21), (2, 22)):
        E = smooth_field(nx, seed)
        sim.set_field(E)
        wb = sim.gather("w") if irk == 1 else sim.gather("wb")
        kappa = w_cancellation(sim.inp, sim.gather("v"))
        sim.push(irk)
        out = []
        for e in (eng, ref):
            e.set_electric(E)
            e.interaction_push_particle(irk)
            g = e.particles_download()
            assert np.array_equal(g["x"], sim.gather("x")), irk
            assert np.array_equal(g["v"], sim.gather("v")), irk
            assert_w_close(g["w"], sim.gather("w"), wb, False, kappa)
            out.append(g["w"])
            e.interaction_collect_charge()
        assert np.array_equal(out[0], out[1]), irk
        sim.array(0, 0, "w")[:] = out[0]
        sim.collect_charge()


@pytest.mark.parametrize("mass", [1.0, 4.0, 1.3])
def test_full_f_mass_division(oracle_mod, amd, mass):
    """full-f still divides by the species mass in the v push
    (src/pic1dp_interaction.F90:336-337): true division unless m is a power of two"""
    kw = dict(deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0], species_mass=[mass])
    sim, eng = pair(oracle_mod, amd, nparticle_max=50001, **kw)
    E = smooth_field(sim.inp.nx, 3)
    sim.set_field(E)
    eng.set_electric(E)
    for irk in (1, 2):
        sim.push(irk)
        eng.interaction_push_particle(irk)
        g = eng.particles_download()
        assert np.array_equal(g["v"], sim.gather("v")) and np.array_equal(g["x"], sim.gather("x"))
        sim.collect_charge()
        eng.interaction_collect_charge()
    # and through the whole-step kernels
    sim2, eng2 = pair(oracle_mod, amd, nparticle_max=50001, **kw)
    t, eo, eg = run_both(sim2, eng2, 5)
    assert np.array_equal(eng2.particles_download()["x"], sim2.gather("x")) or \
        np.max(np.abs(eng2.particles_download()["x"] - sim2.gather("x"))) < 1e-9


def test_upload_between_substeps_restarts_cleanly(oracle_mod, amd):
    """particles_upload after an odd number of pushes (half-step set current):
    the uploaded markers become particle_x/v/p/w, tails included"""
    sim, eng = pair(oracle_mod, amd, nparticle_max=30000, species_nparticle_init=[25000], nx=32)
    eng.interaction_push_particle(1)
    n, npv = eng.local_sizes()
    rng = np.random.default_rng(3)
    x, v = rng.uniform(0, sim.inp.lx, n), rng.uniform(-8, 8, n)
    p, w = rng.uniform(0.5, 1.5, n), rng.uniform(-1e-3, 1e-3, n)
    eng.particles_upload(x, v, p, w, np_valid=npv)
    got = eng.particles_download()
    for k, a in zip("xvpw", (x, v, p, w)):
        assert np.array_equal(got[k], a), k
        sim.array(0, 0, k)[:] = a
    sim.collect_charge()
    sim.solve_field()
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    sim.step(2)
    eng.step(2)
    assert abs(eng.field_energy() / sim.field_energy() - 1.0) < ENERGY_RTOL
    assert relerr(eng.energy_sums(), sim.energy_sums()) < 1e-11


# --------------------------------------------------------------------------
# lazy call sites: the reference's push / collect_charge / solve_field sequence
# runs the whole-step kernels; anything that looks in between gets eager memory
# --------------------------------------------------------------------------
def _fresh(amd, monkeypatch, lazy, **kw):
    monkeypatch.setenv("PIC1DP_LAZY_CALLS", "1" if lazy else "0")
    eng = amd.Pic1dp(amd.make_input(**kw))
    eng.particle_load()
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    return eng


@pytest.mark.parametrize("name,kw,linear", STEP_CASES, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_lazy_call_sites_equal_eager_calls(amd, monkeypatch, name, kw, linear):
    """three call sites per sub-step, never looking in between: the lazy engine
    (whole-step kernels) and the eager one (k_push + k_deposit per call) hold
    bit-identical markers after every step when fed the same fields"""
    kw = dict(kw, nparticle_max=N_SMALL, nx=96, linear=linear)
    a = _fresh(amd, monkeypatch, True, **kw)
    b = _fresh(amd, monkeypatch, False, **kw)
    b.set_electric(a.get_field()["electric"])
    a.kernel_stats_enable(True)
    for it in range(3):
        for irk in (1, 2):
            for e in (a, b):
                e.interaction_push_particle(irk)
                e.particle_optimize(irk)
                e.interaction_collect_charge()
                e.field_solve_electric()
            # (field_chargeden is left alone: between the sub-steps of a step whose half-step charge was predicted as six
            # sums ASKING for it makes the library push and deposit the half-step state after all, see pic1dp_hip_get_field)
            Ea = a.get_field(chargeden=False)["electric"]
            assert relerr(b.get_field()["electric"], Ea) < 1e-10
            b.set_electric(Ea)
        ga, gb = a.particles_download(), b.particles_download()
        for k in "xvw":
            assert np.array_equal(ga[k], gb[k]), (k, it)
    # the lazy engine never ran the per-call kernels
    assert a.kernel_stats(1)[1] == 0 and a.kernel_stats(2)[1] == 0
    # one first-sub-step pass (step 1), afterwards its charge is predicted by the previous step's kernel
    assert a.kernel_stats(3)[1] == 1 and a.kernel_stats(4)[1] == 0 and a.kernel_stats(6)[1] == 3


@pytest.mark.parametrize("where", ["after_push1", "after_collect1", "after_solve1", "after_push2"])
def test_lazy_call_sites_materialise_on_inspection(amd, monkeypatch, where):
    """stop the lazy sequence at every point and look: markers, RK backup and what
    follows are exactly the eager engine's"""
    kw = dict(nparticle_max=N_SMALL, nx=96)
    a = _fresh(amd, monkeypatch, True, **kw)
    b = _fresh(amd, monkeypatch, False, **kw)
    b.set_electric(a.get_field()["electric"])
    seq = [("after_push1", lambda e: e.interaction_push_particle(1)),
           ("after_collect1", lambda e: e.interaction_collect_charge()),
           ("after_solve1", lambda e: e.field_solve_electric()),
           ("after_push2", lambda e: e.interaction_push_particle(2))]
    for tag, fn in seq:
        fn(a)
        fn(b)
        if tag == "after_solve1":
            b.set_electric(a.get_field()["electric"])
        if tag == where:
            break
    ga, gb = a.particles_download(), b.particles_download()
    ba, bb = a.particles_download_bak(), b.particles_download_bak()
    for k in "xvw":
        assert np.array_equal(ga[k], gb[k]), k
        assert np.array_equal(ba[k + "b"], bb[k + "b"]), k
    # carry on to the end of the step (a is eager now) and compare again
    rest = [t for t, _ in seq]
    for tag, fn in seq[rest.index(where) + 1:]:
        fn(a)
        fn(b)
        if tag == "after_solve1":
            b.set_electric(a.get_field()["electric"])
    for e in (a, b):
        e.interaction_collect_charge()
        e.field_solve_electric()
    ga, gb = a.particles_download(), b.particles_download()
    for k in "xvw":
        assert np.array_equal(ga[k], gb[k]), k
    assert relerr(a.get_field()["electric"], b.get_field()["electric"]) < 1e-10


def test_lazy_call_sites_field_changes_between_calls(amd, monkeypatch):
    """a field set between push and collect_charge must not leak into the noted
    push: push(irk) uses the field of its own moment, as an eager call does"""
    kw = dict(nparticle_max=N_SMALL, nx=96)
    a = _fresh(amd, monkeypatch, True, **kw)
    b = _fresh(amd, monkeypatch, False, **kw)
    E1, E2 = smooth_field(96, 5), smooth_field(96, 6)
    for e in (a, b):
        e.set_electric(E1)
        e.interaction_push_particle(1)
        e.set_electric(E2)                    # after the push: must not affect it
        e.interaction_collect_charge()
        e.interaction_push_particle(2)        # sees E2
        e.set_electric(E1)
        e.interaction_collect_charge()
    ga, gb = a.particles_download(), b.particles_download()
    for k in "xvw":
        assert np.array_equal(ga[k], gb[k]), k


def test_library_reports_the_bytes_its_kernels_move(amd, monkeypatch):
    """pic1dp_hip_kernel_bytes: what the marker kernel launched last moves per marker -- read and written bytes
    compulsory for its data flow, the carry of -f0'/f0 apart (bench.py prices its roofline on these instead of
    guessing from constants)"""
    def run(**kw):
        eng = amd.Pic1dp(amd.make_input(**dict(dict(nparticle_max=50_001, nx=64), **kw)))
        eng.particle_load()
        eng.interaction_collect_charge()
        eng.field_solve_electric()
        eng.step(3)
        return eng
    eng = run()
    one = eng.kernel_bytes(6)
    assert (one["read"], one["written"], one["carry"]) == (32.0, 24.0, 0.0) and one["name"].startswith("k_step_one")
    assert "one-exp" in one["name"]
    half = eng.kernel_bytes(3)
    assert (half["read"], half["written"], half["carry"]) == (32.0, 0.0, 0.0) and half["name"] == "k_step_half (one-exp -f0'/f0)"
    monkeypatch.setenv("PIC1DP_DLNF0", "ref")          # the reference-order form carries by default
    ref = run().kernel_bytes(6)
    assert ref["carry"] == 16.0 and "one-exp" not in ref["name"]
    monkeypatch.delenv("PIC1DP_DLNF0")
    lin = run(linear=1).kernel_bytes(6)
    assert (lin["read"], lin["written"]) == (32.0, 16.0)          # v is not pushed in a linear run
    ff = run(deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0]).kernel_bytes(6)
    assert (ff["read"], ff["written"], ff["carry"]) == (24.0, 16.0, 0.0)          # no w in a full-f run
    monkeypatch.setenv("PIC1DP_PRED_KIND", "2")
    assert run().kernel_bytes(6)["name"].startswith("k_step_one<sums>")       # six sums in thread-private LDS slots
    monkeypatch.setenv("PIC1DP_PRED_KIND", "3")
    assert run().kernel_bytes(6)["name"].startswith("k_step_sums")            # the large-grid kernel insisted on
    monkeypatch.delenv("PIC1DP_PRED_KIND")
    assert run(nx=1024).kernel_bytes(6)["name"].startswith("k_step_one<sums>")  # the library's choice for one kept mode
    monkeypatch.setenv("PIC1DP_PRED_KIND", "1")
    assert run().kernel_bytes(6)["name"].startswith("k_step_one (")             # the tiles insisted on
    monkeypatch.delenv("PIC1DP_PRED_KIND")
    assert run(nx=1024, nmode=2, modes=[1, 2]).kernel_bytes(6)["name"].startswith("k_step_one (")   # two kept modes: tiles
    eng = run()
    eng.interaction_push_particle(1)
    eng.particles_download()                           # materialised: the eager push kernel ran
    push = eng.kernel_bytes(1)
    assert (push["read"], push["written"]) == (32.0, 24.0) and push["name"] == "k_push"
