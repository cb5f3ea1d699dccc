"""Where the owned reference blocks of a species lie in its packed arrays (pic1dp_amd/csrc/block_layout.hpp): the valid
markers of all blocks first, in block order, their tail slots behind, in block order.  particle_load, the optimisation
events' blocks, their re-pack and both directions of the pass on host copies take their offsets from this one function; an
off-by-one in it is silent until a chain of events with unequal blocks runs.  Host arithmetic, no GPU."""
import pytest

CASES = {
    "one_block": ([40], [25]),
    "three_unequal_blocks_as_an_event_chain_leaves_them": ([100, 100, 101], [61, 97, 12]),
    "a_block_without_markers": ([50, 50, 50], [30, 0, 45]),
    "a_block_without_tail": ([64, 64], [64, 10]),
    "all_blocks_empty": ([8, 9, 10], [0, 0, 0]),
}


@pytest.fixture(scope="module")
def probe():
    from pic1dp_amd import probe as p
    p.load()
    return p


@pytest.mark.parametrize("name", sorted(CASES))
def test_valid_spans_tile_the_front_and_tail_spans_the_rest_in_block_order(probe, name):
    alloc, np_ = CASES[name]
    spans, total = probe.host_block_layout(alloc, np_)
    assert total == sum(np_)
    assert len(spans) == len(alloc)
    v_end, t_end = 0, total
    for (voff, n, toff, ntail), na, nb in zip(spans, alloc, np_):
        assert n == nb and ntail == na - nb and ntail >= 0
        assert voff == v_end and toff == t_end      # each span begins where the one of the block before it ends
        v_end, t_end = voff + n, toff + ntail
    assert v_end == total and t_end == sum(alloc)   # [0, sum np) and [sum np, sum alloc), nothing left over


def test_mismatched_or_missing_blocks_are_refused(probe):
    with pytest.raises(ValueError):
        probe.host_block_layout([4, 4], [1])
