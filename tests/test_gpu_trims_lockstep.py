"""The unit charge folded into the step constants (device_math.hpp push_core, kernels_step.hip pred_one_private) through the
ONE-PASS kernels, marker by marker and bit for bit: the whole-step kernels against the materialised sub-steps (whose
kernels keep the reference's trailing `* Z`) and the oracle on the same fields (tests/step_lockstep.py), for a unit species
of charge -1 (the unit instances: dt Z from the host) and of charge -2 (the charge must NOT be folded: the power-of-two
instances, the same bits).  tests/test_gpu_trims_bitwise.py holds the two-pass and sub-step kernels to recorded digests; a
one-pass run is not bit-reproducible from run to run (the order of the charge atomics), so here the yardstick is the
lockstep."""
import numpy as np
import pytest

import step_lockstep as ls
from test_gpu_step_lockstep import kept_modes, loaded_trio

pytestmark = pytest.mark.gpu

# (id, family, input): the private sums (the headline kernel), the tiles, the sums in registers
KERNELS = [
    ("private_sums", "private_sums", dict(nx=96, **kept_modes([1]))),
    ("tiles_two_modes", "tiles", dict(nx=96, **kept_modes([1, 2]))),
    ("register_sums_nx1024", "register_sums", dict(nx=1024, **kept_modes([1]))),
]


@pytest.mark.parametrize("charge", [-1.0, -2.0, 1.0])
@pytest.mark.parametrize("kname,family,kkw", KERNELS, ids=[k[0] for k in KERNELS])
def test_one_pass_kernels_equal_substeps_and_oracle_for_unit_and_other_charges(oracle_mod, amd, probe, monkeypatch, kname, family,
                                                                             kkw, charge):
    """loader markers, an odd count over several workgroups, a perturbation of order 0.2; four steps, three predicted"""
    monkeypatch.delenv("PIC1DP_DLNF0", raising=False)
    kw = dict(kkw, nparticle_max=ls.N_SWEEP, species_charge=[charge])
    a, b, sim = loaded_trio(oracle_mod, amd, monkeypatch, family, {}, **kw)
    E = a.get_field(chargeden=False)["electric"]
    assert 0.02 < np.max(np.abs(E)) < 10.0, np.max(np.abs(E))
    v0 = ls.valid(a, 0)["v"]
    ls.lockstep(a, b, 4, 1, sim, probe)
    ls.assert_family_ran(a, family, 4, 1, None)
    assert np.max(np.abs(ls.valid(a, 0)["v"] - v0)) > 1e-3          # accelerated
