"""What every CALL of the call sites launches, scenario by scenario: the launch counts of every marker kernel and of the
counters beside them (kernel_stats rows 0-7, 10, 11) and the name and bytes of the whole-step kernels launched last
(kernel_bytes 3 / 4 / 6), read after every call of a fixed script -- not once at its end, as tests/test_gpu_step_launches.py
does -- against tests/golden/call_site_launches.json, recorded from the library as it stood before the call sites'
decisions moved into call_plan.cpp (tests/golden/gen_call_site_launches.py, on a GPU).  The numbers are that library's, not
derived here: which call launches what is pinned.  nx 32 and 1001 markers (odd, below one workgroup), 3001 / 2001 where an
optimisation event needs them; one engine per scenario.

The scenarios: four time steps through the six calls under every setting that changes what they launch, and every
intruder at every boundary of the third step (B0 in front of its push(1), B1 ... B5 behind its first ... fifth call).  A
bare push(2) intrudes only where a push(1) of this step has gone before it (B1, B2, B3: at B2 it is the push(2) without the
half step's solve_field) -- anywhere else it reads an RK base that no push(1) has written, memory the library never
initialised, and what the markers do then is nobody's contract (tests/call_sequences.py rules it out the same way)."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "call_site_launches.json")
ROWS = (0, 1, 2, 3, 4, 5, 6, 7, 10, 11)
ENV = ("PIC1DP_FUSE_SOLVE", "PIC1DP_PRED_KIND", "PIC1DP_PREDICT", "PIC1DP_CALL_PAIR", "PIC1DP_LAZY_CALLS", "PIC1DP_TAIL")
BASE = dict(nx=32, nparticle_max=1001, dt=0.05, ntime_max=100000, time_max=1000.0, output_interval=0.0)
OPT = dict(nparticle_max=3001, species_nparticle_init=[2001], nv=64, nmerge=1, tmerge=[0.12], thshmerge=[0.3])
STEPS = 4
INTRUDED_STEP = 2      # (the third: the pair path is in its steady state by then)


class Watch:
    """the engine's calls, each followed by an observation"""

    def __init__(self, e):
        self.e, self.calls, self.bytes = e, [], []

    def __call__(self, label, fn, *args):
        """[label, refused, the launches of ROWS, index of the kernel_bytes observation]; fn's result"""
        refused, out = 0, None
        try:
            out = fn(*args)
        except RuntimeError as err:    # (a refusal is an observation too: recorded, and the script goes on;
            refused = getattr(err, "code", 0)              # anything but the library's ARG / STATE ends the scenario)
            if refused not in (1, 4):
                raise
        e = self.e
        e.sync()
        b = [[e.kernel_bytes(w)[n] for n in ("read", "written", "carry", "name")] for w in (3, 4, 6)]
        if b not in self.bytes:
            self.bytes.append(b)
        self.calls.append([label, refused] + [e.kernel_stats(r)[1] for r in ROWS] + [self.bytes.index(b)])
        return out


def collect(w):
    w("collect", w.e.interaction_collect_charge)


def collect_exact(w):
    limbs = w("charge_local_exact", w.e.charge_local_exact)
    w("charge_reduced_exact", w.e.charge_reduced_exact, limbs)


def collect_split(w):
    charge = w("charge_local", w.e.charge_local)
    w("charge_reduced", w.e.charge_reduced, charge)


# -- the intruders: what comes between two of the six calls ----------------------------------------------------------------
def _set_electric(w):
    f = w("get_field(False)", w.e.get_field, False)
    w("set_electric", w.e.set_electric, f["electric"])


def _set_chargeden(w):
    f = w("get_field(True)", w.e.get_field, True)
    w("set_chargeden", w.e.set_chargeden, f["chargeden"])


INTRUDERS = {
    "get_field_E": lambda w: w("get_field(False)", w.e.get_field, False),
    "get_field_cd": lambda w: w("get_field(True)", w.e.get_field, True),
    "download": lambda w: w("particles_download", w.e.particles_download, 0),
    "set_electric": _set_electric,
    "set_chargeden": _set_chargeden,
    "field_energy": lambda w: w("field_energy", w.e.field_energy),
    "output_all": lambda w: w("output_all", w.e.output_all),
    "step": lambda w: w("step(1)", w.e.step, 1),
    "substep": lambda w: w("substep(1)", w.e.substep, 1),
    "solve_again": lambda w: w("solve", w.e.field_solve_electric),
    "collect_again": lambda w: w("collect", w.e.interaction_collect_charge),
    "push2": lambda w: w("push(2)", w.e.interaction_push_particle, 2),
}
PLACES = {name: ((1, 2, 3) if name == "push2" else (0, 1, 2, 3, 4, 5)) for name in INTRUDERS}


def six_calls(collect=collect, before=None, intruder=None, at=None, optimize=False):
    """STEPS time steps through push(1), collect, solve, push(2), collect, solve.  before(w, step, boundary) turns knobs; the
    intruder comes at boundary `at` of the third step; optimize: particle_optimize behind every push(2), as the
    reference's driver calls it, and the clock moved on behind every step (tmerge 0.12 at dt 0.05: the third step's)"""
    def script(w):
        e = w.e
        for step in range(STEPS):
            for b in range(6):
                if before:
                    before(w, step, b)
                if intruder and step == INTRUDED_STEP and b == at:
                    INTRUDERS[intruder](w)
                if b % 3 == 0:
                    w("push(%d)" % (1 + b // 3), e.interaction_push_particle, 1 + b // 3)
                    if optimize and b == 3:
                        w("optimize", e.particle_optimize, 2)
                elif b % 3 == 1:
                    collect(w)
                else:
                    w("solve", e.field_solve_electric)
            if optimize:        # (the driver's clock: the library compares the event times with it)
                e.set_time(e.itime + 1, e.time + e.inp.dt)
    return script


def switch_at_half_step(knob):
    """behind the collect_charge of the third step's push(1), a half-step field owed for adoption: the other solver /
    transform from there on"""
    def before(w, step, b):
        if step == INTRUDED_STEP and b == 2:
            w(knob + "(1)", getattr(w.e, knob), 1)
    return before


def charge_sum_1(w):
    w("set_charge_sum(1)", w.e.set_charge_sum, 1)


# name: (environment, input keywords, script[, what comes in front of the script])
SCENARIOS = {
    "pair_1": ({"PIC1DP_CALL_PAIR": "1"}, {}, six_calls()),
    "pair_0": ({"PIC1DP_CALL_PAIR": "0"}, {}, six_calls()),
    "lazy_0": ({"PIC1DP_LAZY_CALLS": "0"}, {}, six_calls()),
    "tiles_1_mode": ({"PIC1DP_PRED_KIND": "1"}, dict(nmode=1, modes=[1]), six_calls()),
    "tiles_2_modes": ({"PIC1DP_PRED_KIND": "1"}, dict(nmode=2, modes=[1, 2]), six_calls()),
    "predict_0": ({"PIC1DP_PREDICT": "0"}, {}, six_calls()),
    "charge_sum_1_collect": ({}, {}, six_calls(), charge_sum_1),
    "charge_sum_1_split_exact": ({}, {}, six_calls(collect_exact), charge_sum_1),
    "split_six_sums": ({}, {}, six_calls(collect_split)),
    "split_tiles": ({"PIC1DP_PRED_KIND": "1"}, dict(nmode=1, modes=[1]), six_calls(collect_split)),
    "solver_1_at_half_step": ({}, {}, six_calls(before=switch_at_half_step("set_field_solver"))),
    "transform_1_at_half_step": ({}, {}, six_calls(before=switch_at_half_step("set_field_transform"))),
    "optimisation_at_push_2": ({}, OPT, six_calls(optimize=True)),
}
for _name in INTRUDERS:
    for _at in PLACES[_name]:
        SCENARIOS["%s_at_B%d" % (_name, _at)] = ({}, {}, six_calls(intruder=_name, at=_at))


def observe(amd, setenv, delenv, name):
    """the scenario's engine call by call: {"calls": [[label, refused, launches of ROWS ..., bytes index]], "bytes":
    [[read, written, carry, name] of kernel_bytes 3, 4, 6, as first seen]}"""
    env, kw, script = SCENARIOS[name][:3]
    for k in ENV:
        delenv(k)
    for k, v in env.items():
        setenv(k, v)
    e = amd.Pic1dp(amd.make_input(**dict(BASE, **kw)))
    try:
        e.particle_load()
        e.kernel_stats_enable(True)
        w = Watch(e)
        for prepare in SCENARIOS[name][3:]:
            prepare(w)
        w("collect", e.interaction_collect_charge)
        w("solve", e.field_solve_electric)
        script(w)
        return {"calls": w.calls, "bytes": w.bytes}
    finally:
        e.close()


def encoded(obs, pool):
    """an observation as the table stores it, one string per call: "label[ !refusal code][ row[*n]]...[ @k]" -- the rows of
    ROWS that this call raised (by n where n is not 1; the counts only grow), and, where kernel_bytes 3 / 4 / 6 changed with
    this call, their place k in the table's pool of such observations (appended to the pool when new)"""
    out, before, shown = [], [0] * len(ROWS), None
    for call in obs["calls"]:
        label, refused, counts, b = call[0], call[1], call[2:-1], obs["bytes"][call[-1]]
        words = [label] + (["!%d" % refused] if refused else [])
        for row, was, now in zip(ROWS, before, counts):
            assert now >= was
            if now != was:
                words.append("%d" % row if now == was + 1 else "%d*%d" % (row, now - was))
        if b != shown:
            if b not in pool:
                pool.append(b)
            words.append("@%d" % pool.index(b))
        out.append(" ".join(words))
        before, shown = counts, b
    return out


def written(calls, first):
    """a scenario as the table writes it: its calls joined, the ones it begins with like the table's first scenario as "^n" """
    n = 0
    while first is not None and n < min(len(calls), len(first)) and calls[n] == first[n]:
        n += 1
    return "; ".join(calls) if n < 2 else "; ".join(["^%d" % n] + calls[n:])


def recorded(golden, name):
    """the calls of a scenario of the table"""
    calls = golden["scenarios"][name].split("; ")
    if calls[0].startswith("^"):
        calls = golden["scenarios"][next(iter(golden["scenarios"]))].split("; ")[:int(calls[0][1:])] + calls[1:]
    return calls


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_every_scenario_is_recorded(golden):
    assert set(golden["scenarios"]) == set(SCENARIOS)
    assert len(SCENARIOS) == 13 + 11 * 6 + 3


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_every_call_launches_what_it_did(amd, monkeypatch, golden, name):
    pool = [b for b in golden["bytes"]]
    got = encoded(observe(amd, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False), name), pool)
    want = recorded(golden, name)
    assert [c.split(" ")[0] for c in got] == [c.split(" ")[0] for c in want]
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, "call number, what it raised, what is recorded: %r" % bad[:4]
    assert pool == golden["bytes"], "kernel_bytes the recording never saw: %r" % pool[len(golden["bytes"]):]
