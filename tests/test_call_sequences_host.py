"""Census of the call sequences tests/test_gpu_call_sequences.py runs by default, from the generator alone
(tests/call_sequences.py; no GPU): what the default seeds of every mode cover.  These are conditions on the test's INPUTS --
a change to the generator that loses a (read-only intruder, boundary) pair fails here, not silently on the GPU."""
import collections

import pytest

import call_sequences as CS


def default_sequences(mode):
    return [CS.sequence(seed, mode) for seed in range(CS.DEFAULT_SEEDS[mode])]


def census(mode):
    """Counter of (kind, place) over the read-only intruders of the mode's default seeds; the checkpoint counts under
    "restart" or "refused", whichever it expects"""
    count = collections.Counter()
    for seq in default_sequences(mode):
        for kind, place, args, _ in CS.intrusions(seq):
            count[(args["expect"] if kind == "checkpoint" else kind, place)] += 1
    return count


def test_no_more_than_twelve_seeds_per_mode_and_no_fewer_than_the_deck_and_the_references_need():
    for mode in CS.MODES:
        n = CS.DEFAULT_SEEDS[mode]
        assert n <= 12 and n == CS.seeds_needed(mode)
        assert len(CS._deck(mode, 0)) == CS.NCARDS
        by_deck = -(-CS.NCARDS // CS.MAX_CARDS)                 # the smallest n whose hands hold the deck
        by_references = -(-len(CS.REFERENCED) * len(CS.PLACES) // CS.reference_quota(mode))
        assert (by_deck - 1) * CS.MAX_CARDS < CS.NCARDS <= by_deck * CS.MAX_CARDS
        assert (by_references - 1) * CS.reference_quota(mode) < len(CS.REFERENCED) * len(CS.PLACES)
        assert n == max(by_deck, by_references)
    assert CS.DEFAULT_SEEDS == {"tiles": 7, "sums": 7, "exact": 5}


@pytest.mark.parametrize("mode", CS.MODES)
def test_every_pair_of_a_referenced_kind_and_a_place_meets_its_reference(mode):
    """moments, power and their exact kinds are held against the fsum / Python-integer references at chosen intrusions only
    (at most MAX_REFERENCES evaluations per seed): over the default seeds, at every boundary and at P at least once each"""
    covered = collections.Counter()
    for seed in range(CS.DEFAULT_SEEDS[mode]):
        chosen, missing = CS.referenced(seed, mode)
        assert not missing, (mode, missing)
        assert len(chosen) <= CS.reference_quota(mode)
        assert len(chosen) * (1 if mode == "exact" else 2) <= CS.MAX_REFERENCES
        found = CS.intrusions(CS.sequence(seed, mode))
        for i in chosen:
            assert found[i][0] in CS.REFERENCED
            covered[(found[i][0], found[i][1])] += 1
    for kind in CS.REFERENCED:
        for place in CS.PLACES:
            assert covered[(kind, place)] >= 1, (mode, kind, place)
    print(mode, "referenced (kind: B0 B1 B2 B3 B4 B5 P):")
    for kind in CS.REFERENCED:
        print("  %-20s %s" % (kind, " ".join("%2d" % covered[(kind, p)] for p in CS.PLACES)))


def test_the_generator_is_pure_and_seeded():
    for mode in CS.MODES:
        assert CS.sequence(3, mode) == CS.sequence(3, mode)
        assert CS.sequence(3, mode)["ops"] != CS.sequence(4, mode)["ops"]


@pytest.mark.parametrize("mode", CS.MODES)
def test_every_read_only_intruder_at_every_boundary_and_at_P(mode):
    count = census(mode)
    for kind in CS.READ_ONLY:
        if kind == "checkpoint":
            continue
        for place in CS.PLACES:
            assert count[(kind, place)] >= 1, (mode, kind, place)
    assert count[("restart", "B0")] >= 2, mode
    for place in CS.PLACES[1:]:
        assert count[("refused", place)] >= 1, (mode, place)
    for place in CS.PLACES[1:]:                 # a restart only between time steps
        assert count[("restart", place)] == 0, (mode, place)
    print(mode, "intrusions of the default seeds (kind: B0 B1 B2 B3 B4 B5 P):")
    for kind in CS.READ_ONLY[:-1] + ("restart", "refused"):
        print("  %-20s %s" % (kind, " ".join("%2d" % count[(kind, p)] for p in CS.PLACES)))


@pytest.mark.parametrize("mode", CS.MODES)
def test_every_read_only_intruder_is_directly_followed_by_another(mode):
    followed = collections.Counter()
    for seq in default_sequences(mode):
        for kind, _, _, nxt in CS.intrusions(seq):
            if nxt in CS.READ_ONLY:
                followed[kind] += 1
    for kind in CS.READ_ONLY:
        assert followed[kind] >= 1, (mode, kind)


@pytest.mark.parametrize("mode", CS.MODES)
def test_shares_of_two_species_of_two_virtual_ranks_and_a_device_load(mode):
    seqs = default_sequences(mode)
    n = len(seqs)
    assert 3 * sum(s["nspecies"] == 2 for s in seqs) >= n
    assert 3 * sum(s["npe"] == 2 for s in seqs) >= n
    assert any(s["load"] == "device" for s in seqs) and any(s["load"] == "host" for s in seqs)
    for s in seqs:
        kw = s["kw"]
        assert kw["nparticle_max"] % 2 == 1 and 20001 <= kw["nparticle_max"] <= 30001
        assert kw["nx"] in (32, 48, 64, 96, 100) and (kw["nx_opd"], kw["nv_opd"]) in ((8, 8), (16, 32))
        if s["nspecies"] == 2:
            assert kw["species_nparticle_init"] == [kw["nparticle_max"], 7001]
            assert kw["species_charge"][0] * kw["species_charge"][1] < 0
            assert kw["species_mass"][0] != kw["species_mass"][1] and kw["species_density"][0] != kw["species_density"][1]
            assert any(a["isp"] == 1 for _, _, a, _ in CS.intrusions(s) if "isp" in a)    # products take either species
    tails = [i for s in seqs if s["nspecies"] == 2 for k, _, a, _ in CS.intrusions(s) if k == "gather" and a["isp"] == 1
             for i in a["index"] if i >= 7001]
    assert tails, "no tail slot gathered"


def test_the_pair_path_meets_a_read_only_intruder_behind_its_collect_and_behind_its_solve():
    seqs = [s for s in default_sequences("sums") if s["pair_case"]]
    assert len(seqs) >= 2
    for seq in seqs:
        ops = seq["ops"]
        seen = set()
        for i, (op, args) in enumerate(ops):
            q = args.get("after_quiet")
            if not q or (i > 0 and ops[i - 1][1].get("after_quiet")):     # (the first of a run of read-only intruders)
                continue
            assert op in CS.READ_ONLY and args["at"] == "B%d" % q
            n = 12 + q                          # two whole quiet steps, then push1, collect (and its solve)
            quiet = [o for o, _ in ops[i - n:i]]
            assert quiet == (list(CS.REF) * 3)[:n] and ops[i - n - 1][0] == "pair-setup", (i, quiet)
            seen.add(q)
        assert seen == {2, 3}, seen


@pytest.mark.parametrize("mode", CS.MODES)
def test_the_sequences_are_legal(mode):
    """the model's rules, checked from the op list alone: push2 / substep2 only behind a push1 / substep1 with nothing that
    voids the RK backup in between; state-changing calls never at P; a restart only at B0"""
    for seq in default_sequences(mode):
        rk = False
        for op, args in seq["ops"]:
            if op in ("push2", "substep2"):
                assert rk, (mode, op)
            if op in ("push1", "substep1"):
                rk = True
            elif op in ("push2", "substep2", "step", "optimize", "upload") or (op == "checkpoint" and args["expect"] == "restart"):
                rk = False
            if op == "hostsum":
                assert all(k in CS.READ_ONLY and a["at"] == "P" for k, a in args["inside"])
                assert all(a["expect"] == "refused" for k, a in args["inside"] if k == "checkpoint")
        c_ops = CS.without_read_only(seq["ops"])
        assert not any(op in CS.READ_ONLY for op, _ in c_ops)
        assert [op for op, _ in c_ops] == [op for op, _ in seq["ops"] if op not in CS.READ_ONLY]
