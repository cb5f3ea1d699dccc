"""The call sites' state machine as a pure plan (pic1dp_amd/csrc/call_plan.cpp plan_call): against a table transcribed from
the conditions as capi_step.cpp and the intruding entry points held them before (tests/golden/gen_call_plan.py), through the
probe library; walked completely by a program of its own under the host sanitizers (tests/call_plan_check.cpp); and held to
the launch counts DESIGN.md 0 claims for a time step through the six calls.  No GPU."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pic1dp_amd", "csrc")
REFUSALS = ("None", "NotLoaded", "ChargeWaiting", "IllegalState", "EagerNoted", "WantsExactLocal", "WantsExactReduced", "NeedsExactSum",
            "ReducedWithoutLocal", "NotBetweenSteps", "CheckpointChargeWaiting", "CheckpointPushNoted", "CheckpointInsideStep",
            "CheckpointKeptMode", "PlanTooLong")      # call_plan.hpp enum Refusal, in order
LEGAL_PAIRS = {"Clean/Nothing", "Clean/Scale", "Clean/SumScale", "Clean/PredTiles", "Clean/PredSums", "Push1/Nothing", "Half/Nothing",
               "Half/Scale", "Half/SumScale", "Half/PredTiles", "Half/PredSums", "Half/AdoptHalfField", "HalfPair/AdoptHalfField",
               "HalfPairSolved/Nothing", "Push2/Nothing", "Push2/AdoptHalfField", "Push2Pair/AdoptHalfField", "Push2PairSolved/Nothing"}
# the actions that are a kernel launch (copies, bookkeeping and timer spans are not)
LAUNCHES = {"push_eager_1", "push_eager_1_from_e0", "push_eager_2", "wrap_only", "deposit", "half_pass", "full_pass", "fx_settle",
            "chargeden", "chargeden_sum", "pred_chargeden", "pred_chargeden_summed", "pred_combine", "pred_to_charge", "charge_local",
            "fx_to_rho", "solve_pair", "solve_pred_tiles", "solve_pred_sums", "solve_plain"}
MARKER_LAUNCHES = {"push_eager_1", "push_eager_1_from_e0", "push_eager_2", "wrap_only", "deposit", "half_pass", "full_pass"}


@pytest.fixture(scope="module")
def probe():
    from pic1dp_amd import probe as p
    p.load()
    return p


@pytest.fixture(scope="module")
def table():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "call_plan.json")))


def test_the_enums_are_the_ones_the_table_names(probe, table):
    calls, acts = probe.CALL_KINDS, probe.CALL_ACTS
    assert set(calls) == set(table["groups"]) and len(calls) == 26
    assert tuple(table["acts"]) == acts and LAUNCHES <= set(acts) and tuple(table["refusals"]) == REFUSALS[:-1]
    header = open(os.path.join(CSRC, "call_plan.hpp")).read()

    def enumerators(name):
        body = re.search(r"enum class %s : uint8_t \{(.*?)\n\};" % name, header, re.S).group(1)
        return [w for w in re.findall(r"\b[A-Z]\w*\b", re.sub(r"//[^\n]*", "", body)) if w != "N"]

    for name, want in (("Seq", table["seq"]), ("Owed", table["owed"]), ("Refusal", list(REFUSALS))):
        assert enumerators(name) == want, name
    for name, want in (("Call", calls), ("Act", acts)):      # (the probe's names are the enumerators', in order)
        assert [e.lower() for e in enumerators(name)] == [w.replace("_", "") for w in want], name
    legal = {"%s/%s" % tuple(p) for p in table["pairs"]}
    assert legal == LEGAL_PAIRS and len(legal) == 18


def queries(table, call, cap_name):
    """the queries of a group in the table's order (tests/golden/gen_call_plan.py rows): every legal pair under every
    combination of the flags the call can look at with nothing remembered beside the pair; under one cap set also every
    pair with each of the other memories"""
    import itertools
    names = table["flags"].get(call, [])
    for pair, bits in itertools.product(table["pairs"], itertools.product((0, 1), repeat=len(names))):
        yield pair, {}, dict(zip(names, bits))
    if cap_name == table["variants_under"]:
        for pair, variant in itertools.product(table["pairs"], table["variants"][1:]):
            yield pair, variant, {}


def decoded(table, text, came):
    """an answer of the table (its format: gen_call_plan.py) to a call that came in state `came`, as probe.host_call_plan gives one"""
    head, lst = text.split(" ")
    head, _, bad = head.partition("!")
    acts = []
    for a in table["act_lists"][int(lst)].split():
        i, _, arg = a.partition(":")
        acts.append((table["acts"][int(i)], int(arg or 0)))
    return dict(refusal=table["alphabet"].index(head[0]), refused_after=int(head[1]), bad=(int(bad[0]), int(bad[1])) if bad else (0, 0),
                next=dict(zip(table["state"], [came[n] if ch == "." else int(ch) for n, ch in zip(table["state"], head[2:])])), acts=acts)


def test_every_plan_is_the_transcribed_one(probe, table):
    """every kind of call, from every legal (Seq, Owed) pair, over the moment's flags it can look at, under the caps of nine
    contexts, and with what the machine remembers beside the pair: action list, next state and refusal"""
    seq, owed, abc = table["seq"], table["owed"], table["alphabet"]
    assert set(table["cap_sets"]) >= {"six_sums_one_rank", "tiles", "no_prediction", "exact_charge_sum", "several_ranks", "eager_call_sites"}
    assert all(len(places) == len(table["cap_sets"]) == 9 for places in table["groups"].values())
    bad, rows = [], 0
    for call, cap_name, w in ((call, cap_name, w) for call, places in table["groups"].items() for cap_name, w in zip(table["cap_sets"], places)):
        cs, want = table["cap_sets"][cap_name], table["wants"][w]
        asked = list(queries(table, call, cap_name))
        assert len(asked) >= 18 and 2 * len(asked) == len(want)
        for n, ((sq, ow), variant, fl) in enumerate(asked):
            rows += 1
            state = dict(dict.fromkeys(table["state"], 0), **dict(variant, seq=seq.index(sq), owed=owed.index(ow)))
            got = probe.host_call_plan(call, state, dict(cs["moment"], **fl), cs["caps"])
            expect = decoded(table, table["answers"][abc.index(want[2 * n]) * len(abc) + abc.index(want[2 * n + 1])], state)
            got.pop("invariants_hold")
            if got != expect:
                bad.append((call, cap_name, sq, ow, variant, fl, {k: (got[k], expect[k]) for k in expect if got[k] != expect[k]}))
    assert rows > 10000
    assert not bad, "%d of %d rows differ; (got, transcribed) of the first: %r" % (len(bad), rows, bad[:3])


def test_the_whole_state_space_walked_under_the_host_sanitizers(tmp_path):
    """tests/call_plan_check.cpp, a program of its own, built with AddressSanitizer and UndefinedBehaviorSanitizer (host code
    only; nothing of it touches a GPU): every state reachable from (Clean, Nothing) is legal and holds the invariants, no
    plan refuses with a code the entry points did not have, and the pairs reached are the 18 of kCallStateLegal"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pic1dp_amd_build", os.path.join(ROOT, "pic1dp_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    exe = str(tmp_path / "call_plan_check")
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "call_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("\n0 failed"), r.stdout
    reached = re.search(r"^reachable in all: (\d+) pairs:(.*)$", r.stdout, re.M)
    assert int(reached.group(1)) == 18 and set(reached.group(2).split()) == LEGAL_PAIRS
    assert len(re.findall(r"^\w+: \d+ states, \d+ plans, \d+ refused$", r.stdout, re.M)) == 7


def steady_loop(probe, table, cap_set, steps=3):
    """the plans of the six calls of `steps` time steps behind a first collect_charge and solve_field, the moment's flags as
    a run gives them: the prediction and the predicted field are the markers' from the whole-step kernel that made them to
    the next launch that moves markers or solves a field"""
    cs = table["cap_sets"][cap_set]
    state = dict.fromkeys(table["state"], 0)
    pred = eh = False
    out = []
    for call in ["collect_charge", "solve_field"] + ["push1", "collect_charge", "solve_field", "push2", "collect_charge", "solve_field"] * steps:
        p = probe.host_call_plan(call, state, dict(cs["moment"], pred_usable=int(pred), eh_current=int(eh), modes_current=1), cs["caps"])
        assert p["refusal"] == 0 and p["invariants_hold"] == 1, (call, p)
        names = [a for a, _ in p["acts"]]
        if MARKER_LAUNCHES & set(names):
            pred = any(a == "full_pass" and arg & 8 for a, arg in p["acts"]) and bool(cs["caps"]["predict_capable"])
            eh = False
        if "pred_consumed" in names:
            pred = False
        if "mark_eh_current" in names:
            eh = True
        elif "field_written_by_solve" in names:
            eh = False
        state = p["next"]
        out.append((call, names))
    return out


def test_the_launch_counts_design_0_claims(probe, table):
    """six sums on one rank: a time step through the six calls is two launches with the pair (one marker launch, one pair
    solve; push(1), collect_charge and solve_field of the half step launch nothing), three without"""
    last = steady_loop(probe, table, "six_sums_one_rank")[-6:]
    launches = [[n for n in names if n in LAUNCHES] for _, names in last]
    assert [c for c, _ in last] == ["push1", "collect_charge", "solve_field", "push2", "collect_charge", "solve_field"]
    assert launches == [[], [], [], [], ["full_pass"], ["solve_pair"]]
    assert not any(MARKER_LAUNCHES & set(names) for _, names in last[:3])
    last = steady_loop(probe, table, "six_sums_pair_off")[-6:]
    launches = [n for _, names in last for n in names if n in LAUNCHES]
    assert launches == ["solve_pred_sums", "full_pass", "solve_plain"]


def test_the_plan_is_pure():
    """call_plan.cpp and call_plan.hpp include neither ctx.hpp nor a HIP header, and call no HIP function"""
    for name in ("call_plan.cpp", "call_plan.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', text)
        assert includes and not [i for i in includes if "ctx.hpp" in i or i.startswith("hip/") or "hip_runtime" in i], (name, includes)
        code = re.sub(r"//[^\n]*", "", text)
        assert not re.search(r"\bhip[A-Z]\w*\s*\(|\blaunch_\w+\s*\(|pic1dp_ctx", code), name
    probe_units = open(os.path.join(ROOT, "pic1dp_amd", "build.py")).read()
    assert '"call_plan"' in re.search(r"PROBE_SHARED = \[(.*?)\]", probe_units).group(1)
