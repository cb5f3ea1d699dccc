"""The refusals of the marker products' entry points that need no context (pic1dp_amd/csrc/capi_products.cpp: power_len,
moments_limbs_len, moments_quanta, moments_convert): return code and the whole text of pic1dp_hip_last_error(), written out.
The calls with a context share these checks (which_refusal), so a text that moves here moves there."""
import ctypes as C

import numpy as np

ARG = 1       # PIC1DP_ERR_ARG
RANGE = "%s: which = %d, must be 1 (weights p), 2 (weights w) or 3 (both)"
FULL_F = "%s: which = %d asks for the %s of w (which & 2), but a full-f context (deltaf = 0) has no w"


def inputs(amd):
    df = amd.make_input(nparticle_max=10, nx=16, nx_opd=8, nv_opd=8)
    full = amd.make_input(nparticle_max=10, nx=16, nx_opd=8, nv_opd=8, deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0])
    assert df.deltaf == 1 and full.deltaf == 0
    return df, full


def refused(L, rc, text):
    assert rc == ARG and L.pic1dp_hip_last_error() == text.encode(), (rc, L.pic1dp_hip_last_error())


def test_power_len_refusals(amd):
    L = amd._lib.load()
    df, full = inputs(amd)
    n = C.c_int64(-1)
    for which in (0, 4):
        refused(L, L.pic1dp_hip_power_len(C.byref(df), which, C.byref(n)), RANGE % ("power_len", which))
    refused(L, L.pic1dp_hip_power_len(C.byref(full), 2, C.byref(n)), FULL_F % ("power_len", 2, "plane"))
    refused(L, L.pic1dp_hip_power_len(C.byref(full), 3, C.byref(n)), FULL_F % ("power_len", 3, "plane"))
    refused(L, L.pic1dp_hip_power_len(C.byref(df), 1, None), "power_len: null argument")
    refused(L, L.pic1dp_hip_power_len(None, 1, C.byref(n)), "power_len: null argument")
    df.nx_opd = 0
    refused(L, L.pic1dp_hip_power_len(C.byref(df), 1, C.byref(n)), "power_len: nx_opd = 0, nv_opd = 8: nx_opd >= 1 and nv_opd >= 2 required")
    # which is looked at first, then w of a full-f run, then the grid
    refused(L, L.pic1dp_hip_power_len(C.byref(df), 0, C.byref(n)), RANGE % ("power_len", 0))
    assert n.value == -1
    full.nx_opd = 0
    refused(L, L.pic1dp_hip_power_len(C.byref(full), 2, C.byref(n)), FULL_F % ("power_len", 2, "plane"))


def test_moments_limbs_len_refusals(amd):
    L = amd._lib.load()
    n = C.c_int64(-1)
    for which in (0, 4):
        refused(L, L.pic1dp_hip_moments_limbs_len(which, 16, C.byref(n)), RANGE % ("moments_limbs_len", which))
    refused(L, L.pic1dp_hip_moments_limbs_len(3, 16, None), "moments_limbs_len: null argument")
    refused(L, L.pic1dp_hip_moments_limbs_len(3, 0, C.byref(n)), "moments_limbs_len: nx = 0")
    assert n.value == -1
    # only the range: there is no input to say deltaf = 0, and no output grid
    assert L.pic1dp_hip_moments_limbs_len(2, 16, C.byref(n)) == 0 and n.value == 8 * 16
    assert L.pic1dp_hip_moments_limbs_len(3, 16, C.byref(n)) == 0 and n.value == 16 * 16


def test_moments_quanta_refusals(amd):
    L = amd._lib.load()
    df, full = inputs(amd)
    e = (C.c_int32 * 4)()
    refused(L, L.pic1dp_hip_moments_quanta(None, 0, e), "moments_quanta: null argument")
    refused(L, L.pic1dp_hip_moments_quanta(C.byref(df), 0, None), "moments_quanta: null argument")
    refused(L, L.pic1dp_hip_moments_quanta(C.byref(df), 1, e), "species 1 of 1")
    # no `which`, no output grid: a full-f input and nx_opd = 0 are served
    full.nx_opd = 0
    assert L.pic1dp_hip_moments_quanta(C.byref(full), 0, e) == 0
    df.v_max = 0.0
    refused(L, L.pic1dp_hip_moments_quanta(C.byref(df), 0, e), "moments_quanta: v_max must be positive and finite")


def test_moments_convert_refusals(amd):
    L = amd._lib.load()
    df, full = inputs(amd)
    limbs = np.zeros(16 * 16, dtype=np.int64)
    out = np.full(8 * 16, -1.0)
    lp, op = limbs.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for which in (0, 4):
        refused(L, L.pic1dp_hip_moments_convert(C.byref(df), 0, which, lp, op), RANGE % ("moments_convert", which))
    refused(L, L.pic1dp_hip_moments_convert(C.byref(full), 0, 2, lp, op), FULL_F % ("moments_convert", 2, "planes"))
    refused(L, L.pic1dp_hip_moments_convert(C.byref(full), 0, 3, lp, op), FULL_F % ("moments_convert", 3, "planes"))
    refused(L, L.pic1dp_hip_moments_convert(None, 0, 3, lp, op), "moments_convert: null input")
    refused(L, L.pic1dp_hip_moments_convert(C.byref(df), 0, 3, None, op), "moments_convert: null array")
    refused(L, L.pic1dp_hip_moments_convert(C.byref(df), 0, 3, lp, None), "moments_convert: null array")
    refused(L, L.pic1dp_hip_moments_convert(C.byref(df), 1, 3, lp, op), "species 1 of 1")
    assert np.all(out == -1.0)
    # the output grid is not the moments' business
    df.nx_opd = 0
    assert L.pic1dp_hip_moments_convert(C.byref(df), 0, 3, lp, op) == 0 and not np.any(out)
    assert L.pic1dp_hip_moments_convert(C.byref(full), 0, 1, lp, op) == 0
