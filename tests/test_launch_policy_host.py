"""The launch shape of every marker kernel (pic1dp_amd/csrc/launch_policy.cpp: pure arithmetic on the device's size, the
grid, the marker count and three knobs) against a table recorded from the functions this unit was factored out of."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe():
    from pic1dp_amd import probe as p
    p.load()
    return p


def test_every_launch_shape_equals_the_recorded_one(probe):
    """tests/golden/launch_shapes.json: 16 kernel families (sub-step push with and without the rho tile in both kinds of
    the charge sum, deposit, half, full, full<DIAG>, tiles of 1-3 kept modes, sums with and without an exp, private
    sums), each over three grids of cases: 2 device sizes x 10 grids around the LDS turning points (shapes
    beyond the LDS cap included: returned as they are) x 7 marker counts up to 2.3e9 with nothing asked for by hand, and
    35 settings of the knobs (every threads_req x bpc_req, osub_req 1 / 3 / 100 with five of those pairs) where the work
    clamps the grid and where the resident grid or a multiple of it decides, on a large and on a small device.  Recorded
    from capi_step.cpp as it was before the policy left it.  Every element of every shape is equal."""
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "launch_shapes.json")))
    shapes = [tuple(s) for s in t["shapes"]]
    call, query, out = probe.load().pic1dp_probe_host_launch_shape, probe.LaunchQuery(), (probe.C.c_int64 * 4)()
    ref = probe.C.byref(query)
    assert len(t["families"]) == 16
    checked = 0
    for grid in t["grids"]:
        for fam in t["families"]:
            rows = t["rows"][grid["name"]][fam["name"]]
            assert len(rows) == len(grid["num_cu"]) * len(grid["nx"]) * len(grid["np"]) * len(grid["knobs"])
            for key, value in fam.items():
                if key != "name":
                    setattr(query, key, value)
            i = 0
            for query.num_cu in grid["num_cu"]:
                for query.nx in grid["nx"]:
                    for query.np in grid["np"]:
                        for query.threads_req, query.bpc_req, query.osub_req in grid["knobs"]:
                            assert call(ref, out) == 0
                            if tuple(out) != shapes[rows[i]]:
                                pytest.fail("%s num_cu %d nx %d np %d threads_req %d bpc_req %d osub_req %d: (threads, blocks, "
                                            "lds, resident) = %r, recorded %r" % (
                                                fam["name"], query.num_cu, query.nx, query.np, query.threads_req,
                                                query.bpc_req, query.osub_req, tuple(out), shapes[rows[i]]))
                            i += 1
            checked += i
    assert checked == 16 * (2 * 10 * 7 + 2 * 2 * 35 + 35)


def test_an_unknown_family_is_refused(probe):
    with pytest.raises(ValueError):
        probe.host_launch_shape(family=4, num_cu=8, nx=64, np=1000)
    assert probe.host_launch_shape(family=1, num_cu=256, nx=1024, np=100_000_000, full=1) == (768, 512, 24640, 0)
