"""The share of the marker state a non-temporal one-pass launch keeps in the Infinity Cache
(pic1dp_amd/csrc/launch_policy.hpp stream_plain_chunks), pinned on the host: 256 MiB of state for all species
together, in whole 64-pair chunks (4096 B of x, v, w, p) at the head of each species' slab, each species by its marker
count; none for a plain launch."""
import pytest

CHUNK_BYTES = 4096           # 64 pairs x 32 B of state per marker
BUDGET = (256 << 20) // CHUNK_BYTES


def nchunk(np_):
    return ((np_ >> 1) + 63) >> 6


def test_headline_share_and_c2_keep_256_mib(probe):
    for np_ in (10**8, 12_500_000, 10**7, 9_437_185):
        assert probe.host_plain_chunks(np_, np_) == BUDGET == 65536
        assert BUDGET < nchunk(np_)                  # the rest of the slab still streams non-temporally


def test_a_plain_launch_and_an_empty_species_get_none(probe):
    assert probe.host_plain_chunks(10**8, 10**8, nt=False) == 0
    assert probe.host_plain_chunks(10**8, 0) == 0
    assert probe.host_plain_chunks(0, 0) == 0


@pytest.mark.parametrize("counts", [(10**8, 10**8), (3 * 10**7, 10**7), (10**7, 10**7, 10**7, 10**7), (10**8, 1000)])
def test_species_share_the_budget_by_marker_count(probe, counts):
    total = sum(counts)
    got = [probe.host_plain_chunks(total, n) for n in counts]
    assert BUDGET - len(counts) <= sum(got) <= BUDGET       # never more than the cache, and all of it but the rounding
    for g, n in zip(got, counts):
        assert 0 <= g <= nchunk(n)
        assert abs(g - BUDGET * n / total) <= 1


def test_a_slab_within_the_budget_is_plain_throughout(probe):
    """(only a forced non-temporal launch gets here)"""
    for np_ in (2, 129, 4097, 200_001, 1_000_000):
        assert probe.host_plain_chunks(np_, np_) == nchunk(np_)
