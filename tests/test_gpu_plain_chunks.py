"""A non-temporal one-pass launch keeps the head of the marker slab in the Infinity Cache: the first plain_chunks
64-pair chunks go through plain loads and stores, the chunks behind them through non-temporal ones (kernels_step.hip
chunk_plain; launch_policy.hpp stream_plain_chunks).  A cache policy changes no value: at the smallest marker count at
which the library streams non-temporally AND some chunks stay non-temporal -- 9 600 001 markers, 307 MB of state against
the 288 MiB threshold, 75 000 chunks of which 65 536 are plain; an odd count, so the last marker is workgroup 0's --
the three one-pass kernels against the two-pass engine (PIC1DP_PREDICT=0, kernels this policy does not touch), within the
bounds tests/test_gpu_one_pass.py::test_one_pass_equals_two_passes holds them to."""
import numpy as np
import pytest

from util import relerr

pytestmark = pytest.mark.gpu

N = 9_600_001
NSTEPS = 3


def engine(amd, monkeypatch, predict, kind=None, **kw):
    monkeypatch.setenv("PIC1DP_PREDICT", "1" if predict else "0")
    if kind and predict:
        monkeypatch.setenv("PIC1DP_PRED_KIND", str(kind))
    else:
        monkeypatch.delenv("PIC1DP_PRED_KIND", raising=False)
    e = amd.Pic1dp(amd.make_input(nparticle_max=N, **kw))
    e.particle_load_device(1)
    e.interaction_collect_charge()
    e.field_solve_electric()
    return e


# (id, prediction kind, input): the tiles (k_step_one), the private sums with the solve in the prologue (k_step_one<sums>,
# the headline's kernel) and the six sums in registers (k_step_sums); every mode of the push through the headline's kernel
CASES = [("tiles", 1, dict(nx=96)), ("private_sums", 2, dict(nx=1024)), ("sums", 3, dict(nx=1024)),
         ("private_sums_linear", 2, dict(nx=1024, linear=1)),
         ("private_sums_full_f", 2, dict(nx=1024, deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0]))]


@pytest.mark.parametrize("name,kind,kw", CASES, ids=[c[0] for c in CASES])
def test_plain_head_and_streamed_rest_equal_the_two_pass_engine(amd, probe, monkeypatch, name, kind, kw):
    chunks = probe.host_plain_chunks(N, N)
    assert 0 < chunks < ((N >> 1) + 63) >> 6                # both kinds of chunk are met
    assert 32.0 * N > probe.host_settings()["nt_threshold_full"]   # ... because this launch streams non-temporally
    a = engine(amd, monkeypatch, True, kind, **kw)
    b = engine(amd, monkeypatch, False, **kw)
    a.kernel_stats_enable(True)
    a.step(NSTEPS)
    b.step(NSTEPS)
    assert a.kernel_stats(6)[1] == NSTEPS                   # the one-pass kernel ran every step
    ea, eb = a.energy_history(), b.energy_history()
    assert np.max(np.abs(ea / eb - 1.0)) < 1e-11
    assert relerr(a.get_field_half(), b.get_field_half()) < 1e-11
    ga, gb = a.particles_download(), b.particles_download()
    assert ga["x"].size == gb["x"].size == N
    for k in "xvw":
        assert np.max(np.abs(ga[k] - gb[k])) < 1e-11 * max(1.0, np.max(np.abs(gb[k]))), k
