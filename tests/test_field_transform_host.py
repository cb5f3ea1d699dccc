"""Transform 1 of the mode-filter solve (include/pic1dp_hip.h set_field_transform, the FFT) on the host: which grids it
supports, and that every layer declares the two new entry points."""
import os
import re

import pytest

from conftest import ROOT


@pytest.mark.parametrize("nx", [2, 4, 6, 192, 1000, 1024, 3000, 4096, 8192, 3, 5, 15, 243, 3375])
def test_fft_supports_2_3_5_smooth_grids(amd, nx):
    assert amd.field_transform_supported(nx)
    assert amd.field_transform_supported(nx, 0)


@pytest.mark.parametrize("nx", [7, 14, 97, 8191, 1, 0, -4, 8194, 16384, 3645, 6561, 4375])
def test_fft_rejects_other_grids(amd, nx):
    # other prime factors (7, 97, 8191), beyond [2, 8192], odd above 3375 (3645 = 3^6 5, 6561 = 3^8, 4375 = 5^4 7)
    assert not amd.field_transform_supported(nx)


def test_transform_0_takes_every_grid_and_other_transforms_are_errors(amd):
    assert amd.field_transform_supported(97, 0) and amd.field_transform_supported(8191, 0)
    assert not amd.field_transform_supported(1, 0)
    for t in (2, -1):
        with pytest.raises(amd.Pic1dpError) as e:
            amd.field_transform_supported(64, t)
        assert e.value.code == 1


def test_entry_points_declared_in_every_layer(amd):
    names = ("pic1dp_hip_set_field_transform", "pic1dp_hip_field_transform_supported")
    with open(os.path.join(ROOT, "include", "pic1dp_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "pic1dp_amd", "fortran", "pic1dp_hip_mod.F90")) as f:
        fortran = f.read()
    for n in names:
        assert re.search(r"\bint %s\(" % n, header), n
        assert n in amd._lib.SIGNATURES, n
        assert 'name="%s"' % n in fortran, n
        assert hasattr(amd._lib.load(), n), n
    assert hasattr(amd.Pic1dp, "set_field_transform")
    # the Fortran host reads its own option; the library reads no new environment variable
    with open(os.path.join(ROOT, "pic1dp_amd", "fortran", "pic1dp_host.F90")) as f:
        assert "PIC1DP_FIELD_TRANSFORM" in f.read()
    csrc = os.path.join(ROOT, "pic1dp_amd", "csrc")
    for src in os.listdir(csrc):
        if not src.endswith((".cpp", ".hpp", ".hip")):
            continue
        with open(os.path.join(csrc, src)) as f:
            assert "PIC1DP_FIELD_TRANSFORM" not in f.read(), src
