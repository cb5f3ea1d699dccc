"""The exact charge sum (kind 1 of include/pic1dp_hip.h set_charge_sum) on the GPU: the deposit against the host
restatement (tests/exact_charge.py) bit for bit, independence of launch shape / step mode / API / reduction / rank
split, parity with the oracle, the loud overflow, and kind 0 untouched."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import exact_charge as X
from conftest import ROOT

pytestmark = pytest.mark.gpu


def two_species(nx, deltaf, nparticle_max):
    return dict(nx=nx, deltaf=deltaf, nspecies=2, species_charge=[-1.0, 1.0], species_mass=[1.0, 4.0],
                species_temperature=[1.0, 0.5], species_temperature2=[1.0, 0.5], species_density=[1.0, 1.0],
                species_v0=[0.0, 0.0], iptcldist=0, nparticle_max=nparticle_max,
                species_nparticle_init=[nparticle_max, nparticle_max])


def crafted_markers(inp, e, n, seed):
    rng = np.random.default_rng(seed)
    lx = inp.lx
    x = rng.uniform(-0.25 * lx, 1.25 * lx, n)
    q = rng.normal(0.0, 1.0, n) * 2.0 ** (e + 50)
    special_x = [0.0, -0.0, lx, lx / inp.nx, lx - lx / inp.nx, lx * (1 - 2 ** -52), 0.0, 0.0]
    special_q = [2.0 ** (e + 52), -0.0, 0.0, 1.5 * 2.0 ** e, -2.5 * 2.0 ** e, -(2.0 ** (e + 52)),
                 2.0 ** (e + 3) + 0.5 * 2.0 ** e, 2.0 ** (e + 61)]   # ties at half a quantum; one weight near the headroom
    x[:len(special_x)] = special_x
    q[:len(special_q)] = special_q
    return x, q


@pytest.mark.parametrize("nx", [2, 3, 64, 192, 1024, 4096, 8192])
@pytest.mark.parametrize("deltaf,nspecies", [(1, 1), (0, 2)], ids=["df-1sp", "fullf-2sp"])
def test_exact_deposit_equals_the_host_restatement(amd, nx, deltaf, nspecies):
    n = 20001
    kw = two_species(nx, deltaf, n) if nspecies == 2 else dict(nx=nx, deltaf=deltaf, nparticle_max=n)
    inp = amd.make_input(**kw)
    eng = amd.Pic1dp(inp, device=0)
    es = [amd.charge_quantum(inp, s) for s in range(nspecies)]
    xs, qs = [], []
    for s in range(nspecies):
        x, q = crafted_markers(inp, es[s], n, 100 + nx + s)
        v = np.zeros(n)
        # the deposit weighs w (delta-f) or p (full-f)
        eng.particles_upload(x, v, q if not deltaf else np.ones(n), q if deltaf else np.zeros(n), ispecies=s)
        xs.append(x)
        qs.append(q)
    eng.set_charge_sum(1)
    eng.interaction_collect_charge()
    cd = eng.get_field()["chargeden"]
    want, _, _ = X.exact_chargeden(xs, qs, inp, es)
    assert np.array_equal(cd, want)
    assert eng.kernel_stats(14)[1] == 0


KW2 = dict(nparticle_max=2_000_000, nx=1024)


def run_variant(amd, shape=None, mode=0, api="step", steps=10, kind=1):
    eng = amd.Pic1dp(amd.make_input(**KW2), device=0)
    eng.particle_load()
    eng.set_charge_sum(kind)
    if shape is not None:
        eng.set_launch(*shape)
    eng.set_step_mode(mode)
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    if api == "step":
        eng.step(steps)
    elif api == "substep":
        for _ in range(steps):
            eng.substep(1)
            eng.substep(2)
    else:
        for _ in range(steps):
            for irk in (1, 2):
                eng.interaction_push_particle(irk)
                eng.interaction_collect_charge()
                eng.field_solve_electric()
    f = eng.get_field()
    d = eng.particles_download()
    return dict(E=f["electric"], cd=f["chargeden"], energy=np.array([eng.field_energy()]), x=d["x"], v=d["v"], w=d["w"])


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def test_independent_of_launch_shape_step_mode_and_api(amd, tmp_path):
    base = run_variant(amd)
    for shape in ((64, 1), (256, 2), (1024, 1)):
        assert same(run_variant(amd, shape=shape), base), shape
    assert same(run_variant(amd, mode=1), base)
    assert same(run_variant(amd, api="substep"), base)
    assert same(run_variant(amd, api="calls"), base)
    # the eager call sites in a child process of their own (PIC1DP_LAZY_CALLS is read at create)
    out = str(tmp_path / "eager.npz")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import numpy as np, pic1dp_amd as amd; "
            "import test_gpu_exact_charge as T; r = T.run_variant(amd, api='calls'); np.savez(%r, **r)"
            % (ROOT, os.path.join(ROOT, "tests"), out))
    env = dict(os.environ, PIC1DP_LAZY_CALLS="0")
    subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=300)
    eager = dict(np.load(out))
    assert same(eager, base)


def ranks_pair(amd, kw, reduction, steps):
    """two contexts (ranks 0, 1 of two) in this process, one host thread each for the exchange"""
    engs = [amd.Pic1dp(amd.make_input(**kw), rank=r, nranks=2, device=0) for r in range(2)]
    for e in engs:
        e.particle_load()
        e.set_charge_sum(1)
    if reduction == "xchg":
        h = b"".join(e.xchg_create() for e in engs)
        for e in engs:
            e.xchg_connect(h)
            e.set_allreduce(2)
        errors = []

        def body(e):
            try:
                e.interaction_collect_charge()
                e.field_solve_electric()
                e.step(steps)
                e.sync()
            except BaseException as ex:  # noqa: BLE001
                errors.append(repr(ex))
        ts = [threading.Thread(target=body, args=(e,)) for e in engs]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
    else:  # the host owns the sum: the split-phase calls, summed in numpy
        def collect():
            limbs = [e.charge_local_exact() for e in engs]
            tot = limbs[0] + limbs[1]
            for e in engs:
                e.charge_reduced_exact(tot)
        collect()
        for e in engs:
            e.field_solve_electric()
        for _ in range(steps):
            for irk in (1, 2):
                for e in engs:
                    e.interaction_push_particle(irk)
                collect()
                for e in engs:
                    e.field_solve_electric()
    out = []
    for e in engs:
        f = e.get_field()
        out.append(dict(E=f["electric"], cd=f["chargeden"], energy=np.array([e.field_energy()])))
    for e in engs:
        e.close()
    return out


def test_ranks_split_against_virtual_ranks(amd):
    kw = dict(nparticle_max=400_001, nx=256)
    steps = 10
    eng = amd.Pic1dp(amd.make_input(**kw), npe=2, device=0)
    eng.particle_load()
    eng.set_charge_sum(1)
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    eng.step(steps)
    f = eng.get_field()
    base = dict(E=f["electric"], cd=f["chargeden"], energy=np.array([eng.field_energy()]))
    eng.close()   # (at most two contexts at a time: more share hardware queues, test_gpu_exchange.py)
    for reduction in ("host", "xchg"):
        for r in ranks_pair(amd, kw, reduction, steps):
            assert same(r, base), reduction
    # a one-rank RCCL communicator against none
    kw1 = dict(nparticle_max=400_001, nx=256)
    a = amd.Pic1dp(amd.make_input(**kw1), device=0)
    b = amd.Pic1dp(amd.make_input(**kw1), device=0)
    b.comm_available()
    b.comm_init(b.comm_unique_id())
    for e in (a, b):
        e.particle_load()
        e.set_charge_sum(1)
        e.interaction_collect_charge()
        e.field_solve_electric()
        e.step(steps)
    fa, fb = a.get_field(), b.get_field()
    assert np.array_equal(fa["electric"], fb["electric"]) and np.array_equal(fa["chargeden"], fb["chargeden"])


def test_parity_with_the_oracle(amd, oracle_mod):
    kw = dict(nparticle_max=1_000_000, nx=192)
    steps = 40
    sim = oracle_mod.Sim(oracle_mod.make_input(**kw))
    assert sim.load() == 0
    sim.collect_charge()
    sim.solve_field()
    e_o = [sim.field_energy()]
    for _ in range(steps):
        sim.step(1)
        e_o.append(sim.field_energy())
    eng = amd.Pic1dp(amd.make_input(**kw), device=0)
    eng.particle_load()
    eng.set_charge_sum(1)
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    e0 = eng.field_energy()
    eng.step(steps)
    e_g = np.concatenate([[e0], eng.energy_history()])
    assert np.max(np.abs(e_g / np.array(e_o) - 1.0)) < 1e-10


def test_overflow_is_loud_and_recoverable(amd):
    n = 4001
    inp = amd.make_input(nx=64, nparticle_max=n)
    e = amd.charge_quantum(inp, 0)
    eng = amd.Pic1dp(inp, device=0)
    x = np.linspace(0.0, inp.lx, n, endpoint=False)
    w = np.full(n, 2.0 ** (e + 40))
    w[17] = 2.0 ** (e + 63)          # beyond the 2^10 headroom of the quantum
    eng.particles_upload(x, np.zeros(n), np.ones(n), w)
    eng.set_charge_sum(1)
    eng.interaction_collect_charge()
    with pytest.raises(amd.Pic1dpError) as ex:
        eng.get_field()
    assert ex.value.code == 1 and "species 0" in str(ex.value)
    assert eng.kernel_stats(14)[1] > 0
    w[17] = 2.0 ** (e + 40)
    eng.particles_upload(x, np.zeros(n), np.ones(n), w)
    eng.interaction_collect_charge()
    cd = eng.get_field()["chargeden"]
    want, _, _ = X.exact_chargeden([x], [w], inp, [e])
    assert np.array_equal(cd, want)


def test_default_is_kind_0_and_switching_back_restores_it(amd):
    kw = dict(nparticle_max=400_001, nx=1024)
    a = amd.Pic1dp(amd.make_input(**kw), device=0)
    b = amd.Pic1dp(amd.make_input(**kw), device=0)
    pk = a.predict_kind()
    for e in (a, b):
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()
    b.set_charge_sum(1)
    assert b.predict_kind() == 0
    b.step(3)
    with pytest.raises(amd.Pic1dpError):
        b.charge_local()
    b.set_charge_sum(0)
    assert b.predict_kind() == pk
    a.step(3)
    b.step(5)
    a.step(5)
    ea, eb = a.energy_history(), b.energy_history()
    assert np.max(np.abs(ea / eb - 1.0)) < 1e-10
