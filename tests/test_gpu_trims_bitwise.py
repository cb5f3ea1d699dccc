"""The result-preserving strength reductions of the shared per-marker functions (device_math.hpp: x / lx in two operations
where the host proves them, locate without floor, the unit charge folded into the step constants) against the bits of the
commit before them: with the exact charge sum a run is bit-reproducible, and tests/golden/trims_digests.json holds the
digests of the marker state that commit produced (tests/gen_trims_digests.py recorded them)."""
import json

import pytest

import gen_trims_digests as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(G.GOLDEN) as f:
        rec = json.load(f)
    assert rec["steps"] == list(G.STEPS)
    assert rec["lx"] == {k: float(v).hex() for k, v in G.LX.items()}   # the very box lengths, to the bit
    return rec["digests"]


@pytest.mark.parametrize("path", G.PATHS)
@pytest.mark.parametrize("shape,lx", G.CASES)
def test_digests_after_1_2_20_steps_are_the_parents(amd, golden, shape, lx, path):
    """k_step_half / k_step_full<EXACT> (step()) and the sub-step kernels (substep(1), substep(2)) after 1, 2 and 20 steps:
    200 001 markers / nx 64, 65 537 markers / nx 8 with charges -1 and +1, one species of charge -2 (no folding); the box
    2 pi / 0.36, 4 pi, and one whose two-operation quotient is not proven (five operations)"""
    want = golden["%s/%s/%s" % (shape, lx, path)]
    got = G.run_case(amd, shape, lx, path)
    for n, g, w in zip(G.STEPS, got, want):
        assert g == w, "after %d steps" % n
