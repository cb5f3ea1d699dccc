"""The host side of the exact diagnostics sum (kind 1 of set_diag_sum): the quanta from the input
alone, the conversion of limbs, the quantisation of a term against the numpy restatement (tests/diag_exact.py).  No
device."""
import math

import numpy as np
import pytest

import diag_exact as dx


@pytest.fixture(scope="module")
def amd():
    import pic1dp_amd
    return pic1dp_amd


TWO = dict(nspecies=2, species_charge=[-1.0, 1.0], species_mass=[1.0, 4.0], species_temperature=[1.0, 0.5],
           species_temperature2=[1.0, 0.5], species_density=[1.0, 1.0], species_v0=[0.0, 0.0], iptcldist=0)


def test_quanta_do_not_depend_on_the_marker_counts_a_process_holds(amd):
    """two inputs that differ only in the markers a process stores (nparticle_max): the same six quanta -- what every
    rank, and a one-GPU run of the same input, derives without a collective"""
    a = amd.make_input(nparticle_max=8200, species_nparticle_init=[4099, 4099], **TWO)
    b = amd.make_input(nparticle_max=4099, species_nparticle_init=[4099, 4099], **TWO)
    assert [amd.diag_quanta(a, s) for s in range(2)] == [amd.diag_quanta(b, s) for s in range(2)]
    assert amd.diag_quanta(a, 0) != amd.diag_quanta(a, 1)      # (the heavy species' higher peak: its own bound)


@pytest.mark.parametrize("kw", [dict(), dict(v_max=8.0), dict(v_max=7.3, lx=17.0), dict(v_max=0.5, nparticle_max=1000),
                                dict(deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0]), TWO],
                         ids=["default", "vmax8", "vmax7.3", "vmax0.5", "fullf", "two"])
def test_quanta_against_their_bounds(amd, kw):
    inp = amd.make_input(**kw)
    for s in range(inp.nspecies):
        e = amd.diag_quanta(inp, s)
        kb = amd.charge_quantum(inp, s) + 52           # |p|, |w| <= B_s <= 2^kb
        kv = math.ceil(math.log2(inp.v_max * inp.v_max))
        assert 2.0 ** (kv - 1) < inp.v_max ** 2 <= 2.0 ** kv
        bounds = [0, kb, kb]
        for k in range(3):
            assert e[k] <= bounds[k] - 40
        assert e[3:] == [kv - 52, kv + kb - 52, kv + kb - 52]


def test_quanta_reject_bad_arguments(amd):
    inp = amd.make_input()
    for s in (-1, inp.nspecies, 9):
        with pytest.raises(amd.Pic1dpError) as ex:
            amd.diag_quanta(inp, s)
        assert ex.value.code == 1
    inp.abi_version += 1
    with pytest.raises(amd.Pic1dpError) as ex:
        amd.diag_quanta(inp, 0)
    assert ex.value.code == 1


def test_convert_of_hand_made_limbs(amd):
    inp = amd.make_input(nx_opd=3, nv_opd=2)
    nxv = 6
    e = amd.diag_quanta(inp, 0)
    rng = np.random.default_rng(5)
    limbs = np.zeros(6 * nxv + 6, dtype=np.int64)
    hi = limbs[: 6 * nxv].reshape(3, 2, nxv)
    hi[:, 0, :] = rng.integers(-2 ** 40, 2 ** 40, (3, nxv))
    hi[:, 1, :] = rng.integers(0, 2 ** 32, (3, nxv))
    hi[0, 0, 0], hi[0, 1, 0] = -5, 7                       # a negative hi
    hi[0, 0, 1], hi[0, 1, 1] = 3, 2 ** 32 + 9              # a lo that was not normalised
    hi[1, 0, 2], hi[1, 1, 2] = 2 ** 30 + 1, 2 ** 31 + 1    # beyond 2^53: the conversion rounds
    hi[1, 0, 3], hi[1, 1, 3] = 2 ** 22, 1                  # 2^54 + 1: a tie broken by the sticky bit below
    hi[2, 0, 4], hi[2, 1, 4] = -(2 ** 22) - 1, 2 ** 31     # -(2^54 + 2^32) + 2^31
    hi[2, 0, 5], hi[2, 1, 5] = 2 ** 21, 1                  # 2^53 + 1: a tie, to even
    limbs[6 * nxv:] = [-(2 ** 35), 12345, 2 ** 29, 2 ** 33 + 1, 0, 2 ** 32 - 1]
    sums, raw = amd.diag_convert(inp, limbs, 0)
    tot = lambda h, l: int(h) * 2 ** 32 + int(l)           # noqa: E731
    for k, name in enumerate(dx.NAMES):
        ints = [tot(hi[k, 0, i], hi[k, 1, i]) for i in range(nxv)]
        want = [math.ldexp(float(n), e[k]) for n in ints]
        assert list(raw[name + "_xv"]) == want, name
        rows = [sum(ints[r * 3:(r + 1) * 3]) for r in range(2)]
        assert list(raw[name + "_v"]) == [math.ldexp(float(n), e[k]) for n in rows], name
    for k in range(3):
        n = tot(limbs[6 * nxv + 2 * k], limbs[6 * nxv + 2 * k + 1])
        assert sums[k] == math.ldexp(float(n), e[3 + k])
    assert any(abs(tot(hi[k, 0, i], hi[k, 1, i])) > 2 ** 53 for k in range(3) for i in range(nxv))
    with pytest.raises(ValueError):
        amd.diag_convert(inp, limbs[:-1], 0)


def test_convert_returns_the_restatement_from_its_own_integers(amd):
    """the numpy restatement's integers, written as limbs, come back as the restatement's doubles"""
    inp = amd.make_input(nx_opd=5, nv_opd=4, nparticle_max=500)
    e = amd.diag_quanta(inp, 0)
    rng = np.random.default_rng(11)
    n = 500
    b = 2.0 ** (amd.charge_quantum(inp, 0) + 52)
    x, v = rng.uniform(0.0, inp.lx, n), rng.normal(0.0, 3.0, n)
    p, w = rng.uniform(0.0, b, n), rng.uniform(-b, b, n)
    ref = dx.exact(x, v, p, w, n - 50, inp.lx, inp.v_max, 5, 4, 1, e)
    assert ref["rejected"] == [0] * 6
    sums, raw = amd.diag_convert(inp, dx.limbs_of(ref["ints"], 20), 0)
    assert np.array_equal(sums, ref["sums"])
    for k in raw:
        assert np.array_equal(raw[k], ref["raw"][k]), k


def test_quantise_agrees_with_the_restatement(amd):
    rng = np.random.default_rng(3)
    for e in (-40, -47, -52, -3):
        q = 2.0 ** e
        ties = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5, 2.0 ** 30 + 0.5, -(2.0 ** 30) - 1.5, 0.0, -0.0,
                         0.49999999999999994, 2.0 ** 43 + 0.5]) * q
        t = np.concatenate([ties, rng.normal(0.0, 1.0, 200) * q * 2.0 ** rng.integers(0, 43, 200)])
        want, kept = dx.quantise(t, e, dx.HIST_LIMIT)
        assert kept.all()
        got = [amd.diag_quantise(a, e) for a in t]
        assert got == [int(a) for a in want]
        assert amd.diag_quantise(2.5 * q, e) == 2 and amd.diag_quantise(3.5 * q, e) == 4      # ties to even
        # the limits: 2^44 quanta of a histogram term, 2^62 of a kinetic term; NaN
        assert amd.diag_quantise((2.0 ** 44 - 1.0) * q, e) == 2 ** 44 - 1
        assert amd.diag_quantise((2.0 ** 44) * q, e, kinetic=True) == 2 ** 44
        assert amd.diag_quantise(-(2.0 ** 61) * q, e, kinetic=True) == -(2 ** 61)
        for bad, kin in ((2.0 ** 44 * q, False), (-(2.0 ** 44) * q, False), (2.0 ** 62 * q, True), (math.nan, False),
                         (math.nan, True), (math.inf, True)):
            with pytest.raises(amd.Pic1dpError) as ex:
                amd.diag_quantise(bad, e, kinetic=kin)
            assert ex.value.code == 1
            assert not dx.quantise([bad], e, dx.KIN_LIMIT if kin else dx.HIST_LIMIT)[1][0]
