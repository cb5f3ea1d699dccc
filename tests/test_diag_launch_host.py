"""The launch shape of output_all's diagnostics passes and the scales of their fixed-point sums (pic1dp_amd/csrc/
launch_policy.cpp diag_launch, tail_sum_blocks, make_dist_scale: what the launchers and the host take their numbers from)
against a table recorded from the launchers' own formulas as they were before they were written down once
(tests/golden/gen_diag_launch.py)."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe():
    from pic1dp_amd import probe as p
    p.load()
    return p


@pytest.fixture(scope="module")
def table():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "diag_launch.json")))


def test_every_diagnostics_pass_has_the_recorded_shape(probe, table):
    """Blocks, threads, LDS copy or straight into memory, dynamic LDS bytes and NT of k_ptcldist (kind 0) and
    k_ptcldist_exact (kind 1): histogram grids on both sides of the FP64 cap, (3 nxo nvo + 3 nvo) 8 <= 150 KiB (64 x 64,
    80 x 79 | 80 x 80, 40 x 200), and of the exact cap, 8 (3 nxo nvo + 8) <= 150 KiB (79 x 80 | 80 x 80); marker counts
    around one workgroup's trip (2048), around the exact kernel's 2^17 markers per workgroup, on both sides of the NT rule
    (32 np > 288 MiB) and 1e8; 8 and 256 CUs."""
    t = table
    assert [64, 64] in t["grids"] and [80, 79] in t["grids"] and [80, 80] in t["grids"] and [40, 200] in t["grids"]
    assert [79, 80] in t["grids"]
    assert t["np"] == [1, 2, 2047, 2048, 2049, 2**17 - 1, 2**17, 2**18 + 1, 9437184, 9437185, 10**8]
    assert t["num_cu"] == [8, 256]
    seen = {0: set(), 1: set()}
    for kind, name in ((0, "fp64"), (1, "exact")):
        rows = t["rows"][name]
        assert len(rows) == len(t["grids"]) * len(t["np"]) * len(t["num_cu"])
        i = 0
        for nxo, nvo in t["grids"]:
            for np_ in t["np"]:
                for cu in t["num_cu"]:
                    got = probe.host_diag_launch(kind, np_, nxo, nvo, cu)[:5]
                    if list(got) != rows[i]:
                        pytest.fail("kind %d grid %d x %d np %d num_cu %d: (blocks, threads, lds, bytes, nt) = %r, recorded %r"
                                    % (kind, nxo, nvo, np_, cu, got, rows[i]))
                    seen[kind].add((got[2], got[4]))
                    i += 1
    assert seen[0] == seen[1] == {(0, 0), (0, 1), (1, 0), (1, 1)}   # both sides of each cap and of the NT rule
    # the two caps lie between these grids
    assert probe.host_diag_launch(0, 2048, 80, 79, 8)[2] == 1 and probe.host_diag_launch(0, 2048, 80, 80, 8)[2] == 0
    assert probe.host_diag_launch(1, 2048, 79, 80, 8)[2] == 1 and probe.host_diag_launch(1, 2048, 80, 80, 8)[2] == 0


def test_the_tail_slots_get_the_recorded_workgroups(probe, table):
    got = [probe.host_diag_launch(0, 1, 16, 16, 8, ntail=n)[5] for n in table["ntail"]]
    assert got == table["tail_blocks"]
    assert got[0] == 0 and max(got) == 1024


def test_the_fixed_point_scales_are_the_recorded_ones(probe, table):
    """make_dist_scale: the verdict (fixed point or double sums) and the exponents of the three planes' scales, for bounds
    that are unknown (0), negative, infinite, beyond every scale, and ordinary; 256 and 1024 threads; deltaf 0 and 1."""
    t = table
    assert t["threads"] == [256, 1024]
    inf = lambda x: float("inf") if x == "inf" else x
    i, verdicts = 0, set()
    for np_ in t["scale_np"]:
        for blocks in t["scale_blocks"]:
            for deltaf in (0, 1):
                for bp, bw in t["bounds"]:
                    for th in t["threads"]:
                        got = probe.host_dist_scale(np_, blocks, deltaf, inf(bp), inf(bw), th)
                        want = t["scale"][i]
                        # (a bound no scale can serve: 2^e itself overflows or underflows, only the verdict is pinned there)
                        if got[0] != want[0] or (max(abs(e) for e in want[1:]) <= 1022 and list(got) != want):
                            pytest.fail("np %d blocks %d deltaf %d bounds (%r, %r) threads %d: %r, recorded %r"
                                        % (np_, blocks, deltaf, bp, bw, th, got, want))
                        verdicts.add(got[0])
                        i += 1
    assert i == len(t["scale"]) and verdicts == {0, 1}
    assert any(w[0] == 0 and 900 < max(abs(e) for e in w[1:]) <= 1022 for w in t["scale"])   # refused, exponents still pinned


def test_an_unknown_kind_is_refused(probe):
    with pytest.raises(ValueError):
        probe.host_diag_launch(2, 1, 16, 16, 8)
