"""Who allocates device and pinned memory in the product library: pic1dp_amd/csrc/device_mem.hpp, and a short list of places
that have a reason each.  A source scan, like the one of the environment variables in tests/test_host_logic.py."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\s*\(")

# file -> calls it may make, and why they are not the context owner's (pic1dp_ctx::mem)
EXCEPTIONS = {
    # the exchange area: fine-grained / uncached allocators with a fall-back to hipMalloc, IPC handles, and a life cycle of
    # its own (connect / disconnect while the context lives): comm_release
    "capi_comm.cpp": {"hipMalloc": 2, "hipFree": 3, "hipHostMalloc": 1, "hipHostFree": 1},
    # the optimisation events' workers: grow-only scratch with per-worker lifetime and streams of their own, grown on the
    # workers' threads (GrowBuf: DevBuf, HostPin); the event's own scratch is the owner's
    "capi_optimize.cpp": {"hipMalloc": 1, "hipFree": 1, "hipHostMalloc": 1, "hipHostFree": 1},
    # particle_load's pinned stage of one block's markers, freed before the call returns (up to GBs: not kept);
    # chain_selftest's scratch: an optional self-test that must not fail create(), freed before it returns;
    # cell_indices' scratch (a debugging call): two buffers sized by the call, freed before it returns
    "capi.cpp": {"hipMalloc": 3, "hipFree": 3, "hipHostMalloc": 1, "hipHostFree": 1},
    # the FFT's plan builder allocates twiddles and index tables; the context adopts them (capi_step.cpp set_field_transform)
    "kernels_fft.hip": {"hipMalloc": 2},
    # the stamp buffer of -DPIC1DP_TUNE_STAMPS builds only (process lifetime, never in the product)
    "kernels_step.hip": {"hipMalloc": 1},
}
PROBE_LIBRARY = ("probe.hip", "optcheck.cpp", "policy_probe.cpp")   # measurement and test support, not the product


def test_every_allocation_of_the_product_has_one_owner():
    csrc = os.path.join(ROOT, "pic1dp_amd", "csrc")
    found = {}
    for path in sorted(glob.glob(os.path.join(csrc, "*.cpp")) + glob.glob(os.path.join(csrc, "*.hpp")) + glob.glob(os.path.join(csrc, "*.hip"))):
        name = os.path.basename(path)
        if name in PROBE_LIBRARY or name == "device_mem.hpp":
            continue
        calls = {}
        for m in CALL.finditer(open(path).read()):
            calls[m.group(1)] = calls.get(m.group(1), 0) + 1
        if calls:
            found[name] = calls
    assert found == EXCEPTIONS, found
    # the owner itself frees what it hands out, device and pinned
    owner = open(os.path.join(csrc, "device_mem.hpp")).read()
    assert {m.group(1) for m in CALL.finditer(owner)} == {"hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree"}


def test_destroy_releases_through_the_owner_alone():
    """pic1dp_hip_destroy holds no list of pointers: it releases the exchange area, the optimisation workers and the owner"""
    src = open(os.path.join(ROOT, "pic1dp_amd", "csrc", "capi.cpp")).read()
    body = src[src.index("int pic1dp_hip_destroy(pic1dp_ctx *c) {"):]
    body = body[:body.index("\n}\n")]
    assert "c->mem.release_all();" in body and "comm_release(c);" in body and "optimize_release(c);" in body
    assert not CALL.search(body)
