"""pic1dp_hip_kernel_stats row by row (pic1dp_amd/csrc/capi_timing.cpp: one table of {timer tag, counter}), and the marker
products that share one device buffer (pic1dp_amd/csrc/capi_products.cpp: moments, exact moments, power) called one after
the other at sizes that make the buffer grow and shrink."""
import numpy as np
import pytest

import moments_reference as MR
import power_reference as PR
from test_gpu_moments import within as moments_within
from test_gpu_power import within as power_within

pytestmark = pytest.mark.gpu

TAG_ONLY = (0, 1, 2, 3, 4, 6)                    # launches: the spans timed under the tag
COUNTER_ONLY = (5, 7, 8, 10, 11, 15, 18)         # ms = 0, no look at the stream
TAG_AND_COUNTER = (16, 17, 19, 20, 21, 22)
SPECIAL = (9, 12, 13, 14)
# launches of every row after the script below, as the library counted them before the table existed
LAUNCHES = {0: 2, 1: 0, 2: 1, 3: 1, 4: 0, 5: 1, 6: 3, 7: 2, 8: 0, 9: 1, 10: 0, 11: 0, 12: 0, 13: 0, 14: 0, 15: 0, 16: 1, 17: 1,
            18: 0, 19: 0, 20: 1, 21: 4, 22: 1}


def test_every_row_of_kernel_stats(amd):
    e = amd.Pic1dp(amd.make_input(nparticle_max=1001, nx=16, deltaf=1))
    try:
        assert e.inp.nspecies == 1
        e.kernel_stats_enable(True)
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()
        e.step(3)
        e.substep(1)
        e.substep(2)
        e.output_all()
        e.moments(0, 3)
        e.moments_exact(0, 3)
        e.power(0, 3)
        n = e.select_count(0, v=(0.0, np.inf))
        got = e.select(0, v=(0.0, np.inf))
        assert 0 < n < 1001 and got["count"] == n and got["index"].size == n
        e.gather(0, [0, 1000, 7, 7, 500])
        rows = {k: e.kernel_stats(k) for k in range(23)}
        print("kernel_stats rows:", rows)
        assert sorted(TAG_ONLY + COUNTER_ONLY + TAG_AND_COUNTER + SPECIAL) == list(range(23))
        assert {k: r[1] for k, r in rows.items()} == LAUNCHES
        for k in TAG_ONLY + TAG_AND_COUNTER:
            assert (rows[k][0] > 0.0) == (LAUNCHES[k] > 0), (k, rows[k])
            assert rows[k][0] >= 0.0
        for k in COUNTER_ONLY:
            assert rows[k][0] == 0.0, (k, rows[k])
        # 9: create()'s self-test of the sums through the matrix unit; 12: passes repeated in doubles; 13: the first species'
        # bound on |q|; 14: no time either
        assert rows[9][0] == 1.0 and rows[12][0] == 0.0 and np.isfinite(rows[13][0]) and rows[14][0] == 0.0
        for which in (-1, 23):
            with pytest.raises(amd.Pic1dpError) as ei:
                e.kernel_stats(which)
            assert "which must be 0..22" in str(ei.value)
            assert amd._lib.load().pic1dp_hip_last_error() == b"which must be 0..22"
        # timers_reset: the times and the launches counted from the spans go, the counters stay
        e.timers_reset()
        after = {k: e.kernel_stats(k) for k in range(23)}
        for k in TAG_ONLY:
            assert after[k] == (0.0, 0), (k, after[k])
        for k in TAG_AND_COUNTER:
            assert after[k] == (0.0, LAUNCHES[k]), (k, after[k])
        for k in COUNTER_ONLY + SPECIAL:
            assert after[k] == rows[k], (k, after[k], rows[k])
    finally:
        e.close()


# ---------------------------------------------------------------------------
# the products' one buffer
# ---------------------------------------------------------------------------
CALLS = (("power", 3), ("moments", 3), ("moments_exact", 3), ("power", 1), ("moments", 2), ("moments_exact", 1), ("power", 3))


def started(amd, n):
    e = amd.Pic1dp(amd.make_input(nparticle_max=n, nx=16, nx_opd=8, nv_opd=8, deltaf=1))
    e.particle_load()
    e.interaction_collect_charge()
    e.field_solve_electric()
    return e


def flat(res):
    """a product's dict as one array: the sets in order, a power set as plane, v-profile, rest"""
    parts = []
    for name in sorted(res):
        r = res[name]
        parts += [r["xv"].ravel(), r["v"], np.array([r["rest"]])] if isinstance(r, dict) else [r.ravel()]
    return np.concatenate(parts)


def products(amd, n):
    """the seven calls on one context, and each of them on a context of its own"""
    e = started(amd, n)
    try:
        g = e.particles_download()
        E = e.get_field()["electric"].copy()
        inp = e.inp
        shared = [getattr(e, name)(0, which) for name, which in CALLS]
    finally:
        e.close()
    fresh = []
    for name, which in CALLS:
        f = started(amd, n)
        try:
            fresh.append(getattr(f, name)(0, which))
        finally:
            f.close()
    return inp, g, E, shared, fresh


@pytest.mark.parametrize("n", [127, 200_001])
def test_products_share_one_buffer(amd, n):
    """127 markers: one wave sweeps them, so the LDS atomics add in a fixed order and every product repeats bit for bit.
    200 001 markers: the exact sums repeat bit for bit; the FP64 sums, on the shared buffer and on one of their own, lie
    within the references' bounds on a sum in any order (the checks of tests/test_gpu_moments.py and tests/test_gpu_power.py)"""
    inp, g, E, shared, fresh = products(amd, n)
    assert g["x"].size == n
    if n > 127:
        mref = MR.reference(g["x"], g["v"], g["p"], g["w"], inp, which=3)
        pref = PR.reference(g["x"], g["v"], g["p"], g["w"], E, inp, which=3)
        assert MR.workgroups(n) == PR.workgroups(n) == 98
    for (name, which), a, b in zip(CALLS, shared, fresh):
        what = "%s(%d)" % (name, which)
        assert sorted(a) == sorted(b) == [s for bit, s in ((2, "pertb"), (1, "total")) if which & bit]
        assert np.any(flat(a) != 0.0), what
        if n == 127 or name == "moments_exact":
            assert flat(a).tobytes() == flat(b).tobytes(), what
            continue
        for res, where in ((a, "shared"), (b, "own")):
            for s in res:
                if name == "moments":
                    moments_within(res[s], mref[s], MR.workgroups(n), what="%s %s %s" % (what, where, s))
                else:
                    power_within(res[s], pref[s], PR.workgroups(n), "%s %s %s" % (what, where, s))
