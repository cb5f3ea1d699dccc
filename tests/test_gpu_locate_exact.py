"""locate (device_math.hpp) on the device, in both forms of its division -- Markstein's five operations, and the two
operations where the host proves them for the box length -- against numpy's x / lx * nx, bit for bit."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# 2 pi / 0.36 (the default), 4 pi, 1, 17, 0.1, 3 * 2^-7 -- and a box whose two-operation quotient is NOT proven
LXS = [2.0 * math.pi / 0.36, 4.0 * math.pi, 1.0, 17.0, 0.1, 3.0 * 2.0 ** -7, float.fromhex("0x1.800000000019fp+3")]
UNPROVEN = LXS[-1]
NXS = [2, 192, 1024, 8192]


def positions(lx, nx):
    """0, -0, subnormals, lx, its predecessor, every cell boundary +- 1 ulp (and the boundary), random ones: < 2^20"""
    rng = np.random.default_rng(1234 + nx)
    edge = np.arange(nx + 1, dtype=np.float64) * lx / nx
    edge = edge[edge <= lx]
    near = np.concatenate([edge, np.nextafter(edge, np.inf), np.nextafter(edge[1:], 0.0)])
    near = near[near <= lx]
    tiny = np.array([0.0, -0.0, 5e-324, 1e-320, 2.2250738585072009e-308, 2.2250738585072014e-308, 1e-300, 2.0 ** -501, 2.0 ** -499])
    x = np.concatenate([tiny, [lx, np.nextafter(lx, 0.0)], near, rng.random(200_000) * lx,
                        lx * 2.0 ** -rng.integers(1, 60, 20_000) * rng.random(20_000)])
    assert x.size <= 2 ** 20
    return x


def reference(x, lx, nx):
    """sx = x / lx * nx; ix = floor(sx) folded into the grid as the kernels fold it; wl = 1 - (sx - ix)"""
    s = x / lx * float(nx)
    fl = np.floor(s)
    ix = fl.astype(np.int64)
    ix[(ix < 0) | (ix >= nx)] = 0      # memory safety only: x = lx lands in cell nx and is folded to cell 0
    return ix.astype(np.int32), 1.0 - (s - fl)


@pytest.mark.parametrize("nx", NXS)
@pytest.mark.parametrize("lx", LXS, ids=lambda v: float(v).hex())
def test_locate_both_forms_equal_numpy_bit_for_bit(probe, lx, nx):
    x = positions(lx, nx)
    want_ix, want_wl = reference(x, lx, nx)
    forms = {}
    for form in (0, 1):
        ix, wl, two = probe.locate(x, lx, nx, form)
        forms[form] = two
        assert np.array_equal(ix, want_ix), (form, x[ix != want_ix][:5])
        assert wl.tobytes() == want_wl.tobytes(), (form, x[wl.view(np.int64) != want_wl.view(np.int64)][:5])
    assert forms[0] == 0                             # the five operations when asked for
    assert forms[1] == (0 if lx == UNPROVEN else 1)  # two where proven (all six of the list), five for the rejected box


def test_locate_nan_folds_to_cell_zero(probe):
    for form in (0, 1):
        ix, wl, _ = probe.locate(np.array([np.nan]), LXS[0], 192, form)
        assert ix[0] == 0 and np.isnan(wl[0])
