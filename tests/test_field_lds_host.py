"""The dynamic LDS and the workgroup size of every one-workgroup field launch (pic1dp_amd/csrc/field_lds.hpp: the layout the
kernel takes its pointers from and its launcher the byte count) against a table recorded from the launchers' own formulas
as they were before the layouts were written down once."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe():
    from pic1dp_amd import probe as p
    p.load()
    return p


def test_every_field_launch_has_the_recorded_bytes_and_threads(probe):
    """tests/golden/field_lds_bytes.json: the plain solves (k_field_solve and its siblings), launch_field_solve_pair with
    the tile prediction (k_field_solve_pair1 where one mode is kept and the tables fit the LDS, k_field_solve_pair
    otherwise) and with the six sums (k_field_solve_pair_sums1, one kept mode, 256 / 512 / 1024 threads), over 13 grids
    (odd ones for the 16-byte alignment of the product rows, both sides of the thread rule and of the tables' fit) x 5
    numbers of kept modes x 4 reference rank counts, with and without the exchange inside the launch; tab_lds by create()'s
    rule, 2 nmode nx 8 <= 96 KiB.  Bytes, threads and the kernel chosen are all equal."""
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "field_lds_bytes.json")))
    assert t["nx"] == [2, 3, 16, 63, 64, 192, 1023, 1024, 1025, 2048, 2049, 4096, 8192]
    assert t["nmode"] == [1, 2, 3, 8, 128] and t["npe"] == [1, 2, 8, 16] and t["xchg"] == [0, 1]
    assert [(f["name"], f["nmode"]) for f in t["families"]] == [
        ("solve", t["nmode"]), ("pair_tiles", t["nmode"]), ("pair_sums", [1])]
    checked, kernels = 0, set()
    for fam in t["families"]:
        rows = t["rows"][fam["name"]]
        assert len(rows) == len(t["nx"]) * len(fam["nmode"]) * len(t["npe"]) * len(t["xchg"])
        i = 0
        for nx in t["nx"]:
            for nm in fam["nmode"]:
                tab_lds = int(2 * nm * nx * 8 <= 96 * 1024)
                for npe in t["npe"]:
                    for xchg in t["xchg"]:
                        got = probe.host_field_lds(fam["family"], nx, nm, npe, tab_lds, xchg, fam["pred_kind"])
                        if list(got) != rows[i]:
                            pytest.fail("%s nx %d nmode %d npe %d tab_lds %d xchg %d: (bytes, threads, kernel) = %r, "
                                        "recorded %r" % (fam["name"], nx, nm, npe, tab_lds, xchg, got, rows[i]))
                        kernels.add(got[2])
                        i += 1
        checked += i
    assert checked == 13 * 4 * 2 * (5 + 5 + 1)
    assert kernels == {0, 1, 2, 3}


def test_an_unknown_field_family_is_refused(probe):
    with pytest.raises(ValueError):
        probe.host_field_lds(2, 64)
    assert probe.host_field_lds(1, 1024, nmode=1, npe=8, tab_lds=1, with_xchg=1, pred_kind=2) == (24960, 256, 3)
