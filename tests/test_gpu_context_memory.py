"""Every allocation path of a context and its one release path, once under the suite: an engine per configuration that
decides what create() allocates (pic1dp_amd/csrc/context_plan.hpp), each made to touch every buffer that is allocated
lazily (pic1dp_amd/csrc/device_mem.hpp), then closed.  Results are not compared here: the parity, one-pass, exact-sum and
output tests do that."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 200_001
# general divisors and the reference's operation order of -f0'/f0: the whole-step kernels carry it between them (Species::t2)
CARRY = dict(species_mass=[1.1], species_temperature=[1.3], species_temperature2=[0.7])

ROWS = [
    ("tiles", dict(pred_kind="1")),
    ("private_sums", dict()),
    ("register_sums", dict(pred_kind="3")),
    ("eight_ranks_order", dict(npe=8)),
    ("charge_sum_exact", dict(charge_sum=1)),
    ("diag_sum_exact", dict(diag_sum=1)),
    ("fft_transform", dict(transform=1)),
]


@pytest.mark.parametrize("name,how", ROWS, ids=[r[0] for r in ROWS])
def test_every_buffer_is_allocated_and_released(amd, monkeypatch, name, how):
    monkeypatch.setenv("PIC1DP_DLNF0", "ref")
    monkeypatch.setenv("PIC1DP_PREDICT", "1")
    if "pred_kind" in how:
        monkeypatch.setenv("PIC1DP_PRED_KIND", how["pred_kind"])
    else:
        monkeypatch.delenv("PIC1DP_PRED_KIND", raising=False)
    e = amd.Pic1dp(amd.make_input(nparticle_max=N, nx=64, **CARRY), npe=how.get("npe", 0))
    try:
        assert e.predict_kind() == (1 if name == "tiles" else 2)
        if "charge_sum" in how:
            e.set_charge_sum(how["charge_sum"])      # d_fx, h_fx_ovf
        if "diag_sum" in how:
            e.set_diag_sum(how["diag_sum"])
        if "transform" in how:
            e.set_field_transform(how["transform"])  # the FFT plan's tables, adopted
        if name == "register_sums":
            e.particle_load_device()                 # d_loadmax
        else:
            e.particle_load()                        # d_stage
        e.interaction_collect_charge()
        e.field_solve_electric()
        e.step(3)                                    # Species::t2 (the carry), the prediction's buffers
        e.substep(1)                                 # the second marker set
        e.substep(2)
        g = e.particles_download()
        e.particles_upload(g["x"], g["v"], g["p"], g["w"])
        e.interaction_collect_charge()
        e.field_solve_electric()
        e.step(2)
        scal, field, dists = e.output_all()          # d_dist, d_diag_part (d_dfx), d_rec, h_pin
        assert np.all(np.isfinite(scal)) and np.all(np.isfinite(field["electric"])) and len(dists) == 1
        for call, which in ((e.moments, 3), (e.moments_exact, 3), (e.power, 3), (e.power, 1), (e.moments, 1)):
            assert len(call(0, which)) == (2 if which == 3 else 1)   # d_prod: grows twice, is reused at smaller sizes
        got = e.select(0, v=(0.0, np.inf))           # buffers that live for the call; the result through h_pin
        assert 0 < got["count"] == got["index"].size < N
        assert e.gather(0, got["index"][:5])["x"].size == 5
        assert e.state_digest().shape == (1, 4)      # d_digest
        ix, cnt = e.cell_indices()                   # scratch taken from and returned to the owner within the call
        assert int(cnt.sum()) == N and ix.size == N
        assert np.isfinite(e.field_energy())
    finally:
        e.close()
