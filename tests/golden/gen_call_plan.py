"""tests/golden/call_plan.json: what every kind of call of the call sites' state machine enqueues and which state follows,
TRANSCRIBED from the functions of pic1dp_amd/csrc/capi_step.cpp and the intruding entry points of capi.cpp, capi_diag.cpp,
capi_checkpoint.cpp, capi_products.cpp and exact_charge.cpp as they stood at the commit before call_plan.cpp took their
conditions over (round 30; cited below by function) -- not from call_plan.cpp.  Each function below is the function of that
name there, its enqueues replaced by a name appended to a list: the names are those of call_plan.hpp's actions, and the
comment beside each says which launch or bookkeeping of the old code it stands for.  tests/test_call_plan_host.py holds
plan_call to the table through the probe library.
    python tests/golden/gen_call_plan.py [out.json]"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

SEQ = ("Clean", "Push1", "Half", "HalfPair", "HalfPairSolved", "Push2", "Push2Pair", "Push2PairSolved")
OWED = ("Nothing", "Scale", "SumScale", "PredTiles", "PredSums", "AdoptHalfField")
LEGAL = {"Clean": ("Nothing", "Scale", "SumScale", "PredTiles", "PredSums"), "Push1": ("Nothing",), "Half": OWED,
         "HalfPair": ("AdoptHalfField",), "HalfPairSolved": ("Nothing",), "Push2": ("Nothing", "AdoptHalfField"),
         "Push2Pair": ("AdoptHalfField",), "Push2PairSolved": ("Nothing",)}                      # ctx.hpp kCallStateLegal
PAIR = ("HalfPair", "HalfPairSolved", "Push2Pair", "Push2PairSolved")
SOLVED = ("HalfPairSolved", "Push2PairSolved")
LZ = dict(Clean=0, Push1=1, Half=2, HalfPair=2, HalfPairSolved=2, Push2=3, Push2Pair=3, Push2PairSolved=3)   # ctx.hpp lz_of
UNPAIRED = dict(HalfPair="Half", HalfPairSolved="Half", Push2Pair="Push2", Push2PairSolved="Push2")
PUSH2_NOTED = dict(Half="Push2", HalfPair="Push2Pair", HalfPairSolved="Push2PairSolved")
STATE = ("seq", "owed", "e_step_start", "cd_kept_mode_only", "adopt_current", "charge_pending", "charge_pending_pred", "call_phase",
         "eh_modes")
# bits of full_pass's argument (call_plan.hpp): E0 = d_E0, Eh = d_E, diag, pred, eh_modes << 4
E0_SAVED, EH_IS_E, DIAG, PRED = 1, 2, 4, 8


class Refused(Exception):
    def __init__(self, why, pair=("Clean", "Nothing")):
        self.why, self.pair = why, pair


class Ctx:
    """the context as far as the old functions looked at it: the state (s), the moment (m), the caps (k); acts: what they enqueued"""

    def __init__(self, state, moment, caps):
        self.s, self.m, self.k, self.acts = dict(state), moment, caps, []
        self.moved = False      # state_version bumped inside this call: pred_fresh / eh_current no longer hold

    def do(self, name, arg=0):
        if name in ("push_eager_1", "push_eager_1_from_e0", "push_eager_2", "deposit", "state_version"):   # enqueue_push / enqueue_deposit: c->state_version++
            self.moved = True
        self.acts.append([name, arg])

    # -- capi_step.cpp ------------------------------------------------------------------------------------------------------
    def set_call_state(self, seq, owed):
        if owed not in LEGAL[seq]:
            raise Refused("IllegalState", (seq, owed))
        if seq != "Clean" and not self.m["lazy_calls"]:
            raise Refused("EagerNoted")
        self.s["seq"], self.s["owed"] = seq, owed

    def set_seq(self, seq):
        self.set_call_state(seq, self.s["owed"])

    def set_owed(self, owed):
        self.set_call_state(self.s["seq"], owed)

    def pred_usable(self):      # pred_fresh && modes_field_version == field_version && predict_capable
        return self.m["pred_usable"] and not self.moved

    def eh_current(self):
        return self.m["eh_current"] and not self.moved

    def adopt_current(self):    # adopt_cd_version == cd_version
        return self.s["adopt_current"]

    def cd_version_bump(self):
        self.do("cd_version")
        self.s["adopt_current"] = False

    def materialize_cd(self):
        pending = self.s["owed"]
        if pending in ("AdoptHalfField", "Nothing"):
            return
        self.set_owed("Nothing")
        if pending == "PredSums":
            self.do("pred_chargeden")           # launch_pred_chargeden(fa, pred_tab, d_pred, nullptr)
            return
        if pending == "PredTiles":
            self.do("pred_combine")             # launch_pred_combine
        self.do("chargeden_sum" if pending == "SumScale" else "chargeden")      # launch_chargeden(fa, pending == SumScale)

    def settle_half_pair(self):
        if self.s["seq"] not in PAIR:
            return
        self.do("save_step_start_field")
        solved = self.s["seq"] in SOLVED
        self.set_seq(UNPAIRED[self.s["seq"]])
        if solved:
            self.do("adopt_half_field")

    def settle_step_start_field(self):
        if not self.s["e_step_start"]:
            return
        self.s["e_step_start"] = False
        self.do("copy_eh_to_e")                 # hipMemcpyAsync(d_E, d_Eh)
        self.do("adopt_half_modes")

    def settle_field_view(self):
        self.settle_step_start_field()
        if self.s["seq"] in SOLVED:
            self.settle_half_pair()

    def rebuild_half_step_chargeden(self):
        if self.m["several_ranks"]:
            return
        if LZ[self.s["seq"]] not in (2, 3):
            return
        self.settle_half_pair()
        if self.s["owed"] == "AdoptHalfField":
            self.set_owed("Nothing")
        push2_was_noted = LZ[self.s["seq"]] == 3
        self.do("push_eager_1_from_e0")         # enqueue_push(c, 1, false, c->d_E0)
        self.set_seq("Clean")
        self.do("deposit")
        if self.m["charge_sum"] == 1:
            self.do("fx_settle")
        self.do("chargeden_sum")                # launch_chargeden(fa, true)
        self.s["cd_kept_mode_only"] = False
        if push2_was_noted:
            self.do("push_eager_2")

    def materialize(self):
        self.settle_half_pair()
        lz = LZ[self.s["seq"]]
        if lz == 0:
            return
        if self.s["owed"] == "AdoptHalfField":
            return self.rebuild_half_step_chargeden()
        self.set_seq("Clean")
        if lz == 1:
            return self.do("push_eager_1")      # enqueue_push(c, 1, false)
        self.do("push_eager_1_from_e0")
        self.do("wrap_only")
        if lz == 3:
            self.do("push_eager_2")

    def require_loaded_keep_lazy(self):
        if not self.m["loaded"]:
            raise Refused("NotLoaded")
        if self.s["charge_pending"]:
            raise Refused("ChargeWaiting")
        self.settle_step_start_field()
        self.materialize_cd()

    def require_loaded(self):
        self.require_loaded_keep_lazy()
        self.materialize()

    def deposit_or_step(self):
        s = self.s
        if s["seq"] == "Push1":
            self.do("save_step_start_field")
            self.do("half_pass")                # step_particles(c, s, false, d_E, d_Eh)
            return self.set_seq("Half")
        if LZ[s["seq"]] == 3:
            if s["seq"] == "Push2Pair":
                self.settle_half_pair()
            self.do("state_version")
            diag = bool(self.k["diag_in_step"] and self.m["output_follows"])
            want = DIAG if diag else PRED       # step_particles(..., diag, !diag)
            if s["seq"] == "Push2PairSolved":
                self.do("swap_eh")
                s["eh_modes"] = 2
                self.do("full_pass", want | (2 << 4))            # E0 = d_E, Eh = d_Eh
                s["e_step_start"] = True
                return self.set_seq("Clean")
            s["eh_modes"] = 1 if (self.k["dft_paths"] and self.m["modes_current"]) else 0
            self.do("full_pass", want | E0_SAVED | EH_IS_E | (s["eh_modes"] << 4))   # E0 = d_E0, Eh = d_E
            return self.set_seq("Clean")
        self.materialize()
        self.do("deposit")

    def pred_to_chargeden(self, defer):         # (f = c->fa: f.chargeden is field_chargeden)
        self.do("pred_consumed")                # c->pred_version = 0
        multi = self.m["several_ranks"]
        if self.m["pred_kind"] == 2:
            self.s["cd_kept_mode_only"] = True
            if defer and not multi and self.k["dft_paths"] and self.m["tab_lds"]:
                return self.set_owed("PredSums")
            if not multi:
                return self.do("pred_chargeden")
            self.do("pred_to_charge")
            self.do("pred_reduce")
            return self.do("pred_chargeden_summed")              # launch_pred_chargeden(f, pred_tab, nullptr, d_charge)
        if defer and not multi and self.k["dft_paths"] and self.k["modes_fit_field_kernel"]:
            return self.set_owed("PredTiles")
        self.do("pred_combine")
        if multi:
            self.do("pred_reduce")
        if defer:
            return self.set_owed("Scale")
        self.do("chargeden")

    def call_phase_collect(self):
        if self.s["call_phase"] in (1, 4):
            self.s["call_phase"] += 1

    def collect_charge(self):                   # pic1dp_hip_collect_charge
        s, m, k = self.s, self.m, self.k
        self.require_loaded_keep_lazy()
        self.call_phase_collect()
        self.cd_version_bump()
        if s["seq"] in PAIR and s["seq"] != "Push2PairSolved":
            self.settle_half_pair()
        if s["seq"] == "Push1" and k["pair_serves_collect"] and self.eh_current():
            s["cd_kept_mode_only"] = True
            s["adopt_current"] = True           # adopt_cd_version = cd_version
            return self.set_call_state("HalfPair", "AdoptHalfField")
        if s["seq"] == "Push1" and self.pred_usable():
            self.do("save_step_start_field")
            self.set_call_state("Half", "Nothing")
            self.do("span_collect")
            self.pred_to_chargeden(bool(m["lazy_calls"]))
            return self.do("span_end")
        s["cd_kept_mode_only"] = False
        if s["owed"] == "AdoptHalfField":
            self.set_owed("Nothing")
        noted = LZ[s["seq"]] in (1, 3)
        if noted:
            self.deposit_or_step()
        self.do("span_collect")
        if not noted:
            self.deposit_or_step()
        if m["charge_sum"] == 1:
            self.do("fx_settle")
        multi = m["fp64_rank_sum"]
        if multi:
            self.do("reduce_charge")
        if m["lazy_calls"]:
            self.set_owed("Scale" if multi else "SumScale")
        else:
            self.do("chargeden" if multi else "chargeden_sum")   # launch_chargeden(fa, !multi)
        self.do("span_end")

    def solve_field(self):                      # pic1dp_hip_solve_field, solve_field_call
        s, k = self.s, self.k
        if s["seq"] == "HalfPair":
            self.set_call_state("HalfPairSolved", "Nothing")
            self.do("call_pair_skip")
            self.field_written_by_solve()
        else:
            self.settle_half_pair()
            if LZ[s["seq"]] in (1, 3):
                self.materialize()
            self.do("span_field")
            pending = s["owed"]
            self.set_owed("Nothing")
            if pending == "AdoptHalfField" and not self.adopt_current():
                pending = "Nothing"
            if pending == "SumScale" and k["pair_in_solve_field"] and s["seq"] == "Clean" and self.pred_usable():
                self.do("solve_pair")
                self.field_written_by_solve()   # pair_solved: field_written, pred_version = 0, mark_eh_current
                self.do("pred_consumed")
                self.do("mark_eh_current")
            else:
                if pending == "AdoptHalfField":
                    self.do("adopt_half_field")
                elif pending == "PredTiles" and k["dft_paths"]:
                    self.do("solve_pred_tiles")
                elif pending == "PredSums" and k["dft_paths"]:
                    self.do("solve_pred_sums")
                else:
                    if pending == "PredSums":
                        self.do("pred_chargeden")
                    if pending == "PredTiles":
                        self.do("pred_combine")
                    self.do("solve_plain", (1 if pending == "SumScale" else 0) | (2 if pending in ("Nothing", "PredSums") else 0))
                self.field_written_by_solve()
            self.do("span_end")
        if s["call_phase"] == 2:                # call_phase_solve
            s["call_phase"] = 3
        elif s["call_phase"] == 5:
            s["call_phase"] = 0

    def field_written_by_solve(self):           # field_written(c, true): versions, and e_step_start = false
        self.do("field_written_by_solve")
        self.s["e_step_start"] = False

    def push(self, irk):                        # pic1dp_hip_push
        s = self.s
        self.require_loaded_keep_lazy()
        if irk == 1 and s["seq"] == "Clean" and self.k["lazy_calls_ok"] and not self.m["optimize_due_any"]:   # lazy_ok
            self.set_seq("Push1")
        elif irk == 2 and LZ[s["seq"]] == 2:
            self.set_seq(PUSH2_NOTED[s["seq"]])
        else:
            self.materialize()
            self.do("push_eager_1" if irk == 1 else "push_eager_2")
        s["call_phase"] = 1 if irk == 1 else 4

    def charge_local(self):                     # pic1dp_hip_charge_local
        s, m = self.s, self.m
        if m["charge_sum"] == 1:
            raise Refused("WantsExactLocal")
        self.require_loaded_keep_lazy()
        if s["seq"] in PAIR and s["seq"] != "Push2PairSolved":
            self.settle_half_pair()
        if s["owed"] == "AdoptHalfField":
            self.set_owed("Nothing")
        if s["seq"] == "Push1" and self.pred_usable():
            self.do("save_step_start_field")
            self.set_seq("Half")
            if m["pred_kind"] == 2:
                self.do("pred_to_charge")
                s["charge_pending_pred"] = True
            else:
                self.do("pred_combine")
            self.do("pred_consumed")
        else:
            s["cd_kept_mode_only"] = False
            self.deposit_or_step()
            self.do("charge_local")             # launch_charge_local
        s["charge_pending"] = True

    def charge_reduced(self):                   # pic1dp_hip_charge_reduced
        s, m = self.s, self.m
        if m["charge_sum"] == 1:
            raise Refused("WantsExactReduced")
        if not s["charge_pending"]:
            raise Refused("ReducedWithoutLocal")
        s["charge_pending"] = False
        self.call_phase_collect()
        self.cd_version_bump()
        if s["charge_pending_pred"]:
            s["charge_pending_pred"] = False
            s["cd_kept_mode_only"] = True
            return self.do("pred_chargeden_summed")
        if m["lazy_calls"]:
            return self.set_owed("Scale")
        self.do("chargeden")

    def charge_local_exact(self):               # pic1dp_hip_charge_local_exact up to the hand-out of the limbs
        if self.m["charge_sum"] != 1:
            raise Refused("NeedsExactSum")
        self.require_loaded_keep_lazy()
        self.s["cd_kept_mode_only"] = False
        self.deposit_or_step()

    def charge_exact_handed_out(self):          # ... and behind it: fx_check passed, c->charge_pending = true
        self.s["charge_pending"] = True

    def charge_reduced_exact(self):             # pic1dp_hip_charge_reduced_exact
        s, m = self.s, self.m
        if m["charge_sum"] != 1:
            raise Refused("NeedsExactSum")
        if not s["charge_pending"]:
            raise Refused("ReducedWithoutLocal")
        s["charge_pending"] = False
        self.call_phase_collect()
        self.cd_version_bump()
        self.do("fx_to_rho")
        if m["lazy_calls"]:
            return self.set_owed("SumScale")
        self.do("chargeden_sum")

    def whole_steps(self, phase):               # pic1dp_hip_step(n > 0) / pic1dp_hip_substep up to the first launch of their own
        self.require_loaded()
        self.s["cd_kept_mode_only"] = False
        self.cd_version_bump()
        self.s["call_phase"] = phase

    # -- the intruders ------------------------------------------------------------------------------------------------------
    def get_field(self, cd):                    # capi.cpp pic1dp_hip_get_field
        self.settle_field_view()
        self.materialize_cd()
        if cd and self.s["cd_kept_mode_only"]:
            self.rebuild_half_step_chargeden()

    def output_all(self, cd):                   # capi_diag.cpp pic1dp_hip_output_all (one rank)
        self.require_loaded()
        self.get_field(cd)

    def set_electric(self):                     # capi.cpp pic1dp_hip_set_electric up to the copy
        self.settle_step_start_field()
        self.settle_half_pair()
        if LZ[self.s["seq"]] in (1, 3):
            self.materialize()

    def set_chargeden(self):                    # capi.cpp pic1dp_hip_set_chargeden
        self.materialize_cd()
        self.settle_half_pair()
        if self.s["owed"] == "AdoptHalfField":
            self.set_owed("Nothing")
        self.cd_version_bump()
        self.s["cd_kept_mode_only"] = False

    def particle_load(self):                    # capi.cpp pic1dp_hip_particle_load, _particle_load_device
        self.materialize_cd()
        if self.s["owed"] == "AdoptHalfField":
            self.rebuild_half_step_chargeden()
        self.set_call_state("Clean", "Nothing")
        self.s["call_phase"] = 0

    def particles_upload(self):                 # capi.cpp pic1dp_hip_particles_upload
        self.materialize_cd()
        if self.m["loaded"]:
            self.materialize()
        self.s["call_phase"] = 0

    def switch_field(self):                     # capi_step.cpp pic1dp_hip_set_field_solver, _set_field_transform
        if self.s["owed"] == "AdoptHalfField" and self.m["field_differs"]:
            self.rebuild_half_step_chargeden()
            self.set_owed("Nothing")

    def between_steps(self):                    # exact_charge.cpp pic1dp_hip_set_charge_sum, capi_diag.cpp pic1dp_hip_set_diag_sum
        s = self.s
        if s["seq"] != "Clean" or s["owed"] != "Nothing" or s["charge_pending"]:
            raise Refused("NotBetweenSteps")

    def checkpoint(self):                       # capi_checkpoint.cpp pic1dp_hip_checkpoint_write up to the file
        s = self.s
        if not self.m["loaded"]:
            raise Refused("NotLoaded")
        if s["charge_pending"]:
            raise Refused("CheckpointChargeWaiting")
        if LZ[s["seq"]] != 0:
            raise Refused("CheckpointPushNoted")
        if s["call_phase"] != 0:
            raise Refused("CheckpointInsideStep")
        self.settle_step_start_field()
        self.materialize_cd()
        if s["cd_kept_mode_only"]:
            return "CheckpointKeptMode"         # (refused behind what has been settled)


CALLS = {
    "push1": lambda c: c.push(1), "push2": lambda c: c.push(2), "collect_charge": Ctx.collect_charge, "charge_local": Ctx.charge_local,
    "charge_reduced": Ctx.charge_reduced, "charge_local_exact": Ctx.charge_local_exact, "charge_exact_handed_out": Ctx.charge_exact_handed_out,
    "charge_reduced_exact": Ctx.charge_reduced_exact, "solve_field": Ctx.solve_field, "markers": Ctx.require_loaded,
    "read_markers": Ctx.materialize,            # particles_download, state_digest, product_begin
    "whole_steps": lambda c: c.whole_steps(0), "substep1": lambda c: c.whole_steps(3), "substep2": lambda c: c.whole_steps(0),
    "read_field": Ctx.settle_field_view,        # pic1dp_hip_field_energy, the power products
    "get_field": lambda c: c.get_field(False), "get_field_cd": lambda c: c.get_field(True),
    "output_all": lambda c: c.output_all(False), "output_all_cd": lambda c: c.output_all(True),
    "write_electric": Ctx.set_electric, "write_chargeden": Ctx.set_chargeden, "replace_markers": Ctx.particle_load,
    "upload_markers": Ctx.particles_upload, "switch_field": Ctx.switch_field, "between_steps": Ctx.between_steps, "checkpoint": Ctx.checkpoint,
}
# which of the moment's flags a kind of call can look at (every other one is held at 0)
FLAGS = {"push1": ("optimize_due_any",), "collect_charge": ("pred_usable", "eh_current", "modes_current", "output_follows"),
         "charge_local": ("pred_usable", "modes_current", "output_follows"), "charge_local_exact": ("modes_current", "output_follows"),
         "solve_field": ("pred_usable",), "switch_field": ("field_differs",)}


def answer(call, state, moment, caps):
    """[refusal, refused_after, the refused pair, the state that follows, the actions]"""
    c = Ctx(state, moment, caps)
    try:
        late = CALLS[call](c)
    except Refused as r:
        return [r.why, 0, list(r.pair), [state[n] for n in STATE], []]
    nxt = dict(c.s)
    if nxt["owed"] != "AdoptHalfField":         # (adopt_cd_version only means something while an adoption is owed)
        nxt["adopt_current"] = False
    return [late or "None", 1 if late else 0, ["Clean", "Nothing"], [nxt[n] for n in STATE], c.acts]


def caps_of(lazy=1, pair=1, pred_kind=2, nmode_one=1, predict=1, charge_sum=0, several=0, dft=1, fuse_output=0):
    """(caps, the context's part of the moment) as step_plan.cpp step_caps derives them (round 27's transcription:
    tests/golden/gen_step_plan.py), for a context whose whole-step kernels run"""
    six = pred_kind == 2 and nmode_one
    capable = charge_sum == 0 and predict and pred_kind != 0 and dft
    caps = dict(dft_paths=dft, six_sums_one_mode=int(bool(six)), modes_fit_field_kernel=1, predict_capable=int(bool(capable)),
                diag_in_step=int(charge_sum == 0 and (fuse_output == 2 or (fuse_output == 1 and not capable))), lazy_calls_ok=lazy,
                pair_serves_collect=int(bool(pair and lazy and not several and capable and six)),
                pair_in_solve_field=int(bool(pair and lazy and dft and capable and six)))
    moment = dict(lazy_calls=lazy, call_pair=pair, loaded=1, several_ranks=several, fp64_rank_sum=int(bool(several and charge_sum == 0)),
                  charge_sum=charge_sum, pred_kind=pred_kind, tab_lds=1)
    return caps, moment


CAP_SETS = {
    "six_sums_one_rank": caps_of(),
    "six_sums_pair_off": caps_of(pair=0),
    "tiles": caps_of(pred_kind=1, nmode_one=0),
    "no_prediction": caps_of(predict=0, fuse_output=1),
    "exact_charge_sum": caps_of(charge_sum=1),
    "several_ranks": caps_of(several=1),
    "eager_call_sites": caps_of(lazy=0),
    "other_solver": caps_of(dft=0),
    "not_loaded": (caps_of()[0], dict(caps_of()[1], loaded=0)),
}
# what the machine remembers beside the pair: nothing (asked under every cap set and every combination of the flags), and
# five other memories (asked under VARIANTS_UNDER with the flags at 0)
VARIANTS = [{}, {"e_step_start": 1, "eh_modes": 2, "cd_kept_mode_only": 1, "call_phase": 1}, {"adopt_current": 1, "call_phase": 2},
            {"charge_pending": 1, "call_phase": 4}, {"charge_pending": 1, "charge_pending_pred": 1, "call_phase": 5},
            {"cd_kept_mode_only": 1, "call_phase": 5}]
VARIANTS_UNDER = "six_sums_one_rank"
PAIRS = [[seq, owed] for seq in SEQ for owed in OWED if owed in LEGAL[seq]]
REFUSALS = ("None", "NotLoaded", "ChargeWaiting", "IllegalState", "EagerNoted", "WantsExactLocal", "WantsExactReduced", "NeedsExactSum",
            "ReducedWithoutLocal", "NotBetweenSteps", "CheckpointChargeWaiting", "CheckpointPushNoted", "CheckpointInsideStep",
            "CheckpointKeptMode")
ACTS = ("save_step_start_field", "adopt_half_field", "adopt_half_modes", "copy_eh_to_e", "push_eager_1", "push_eager_1_from_e0",
        "push_eager_2", "wrap_only", "deposit", "half_pass", "swap_eh", "full_pass", "fx_settle", "reduce_charge", "chargeden",
        "chargeden_sum", "pred_chargeden", "pred_chargeden_summed", "pred_combine", "pred_to_charge", "pred_reduce", "charge_local",
        "fx_to_rho", "solve_pair", "solve_pred_tiles", "solve_pred_sums", "solve_plain", "state_version", "cd_version",
        "field_written_by_solve", "call_pair_skip", "pred_consumed", "mark_eh_current", "span_collect", "span_field", "span_end")
# two characters per row: the answer's index in base len(ALPHABET)
ALPHABET = "".join(chr(c) for c in range(35, 127) if chr(c) != "\\")


def rows(call, cap_name):
    """every query of a (kind of call, cap set) group in the table's order: (state, the moment's flags)"""
    names = FLAGS.get(call, ())
    flags = [dict(zip(names, bits)) for bits in itertools.product((0, 1), repeat=len(names))]
    for (seq, owed), fl in itertools.product(PAIRS, flags):
        yield dict(dict.fromkeys(STATE, 0), seq=seq, owed=owed), fl
    if cap_name == VARIANTS_UNDER:
        for (seq, owed), variant in itertools.product(PAIRS, VARIANTS[1:]):
            yield dict(dict.fromkeys(STATE, 0), seq=seq, owed=owed, **variant), {}


class Pool:
    def __init__(self):
        self.items, self.index = [], {}

    def __call__(self, item):
        if item not in self.index:
            self.index[item] = len(self.items)
            self.items.append(item)
        return self.index[item]


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "call_plan.json")
    assert len(PAIRS) == 18
    act_lists, answers, wants, groups, nrows = Pool(), Pool(), Pool(), {}, 0     # groups: call -> its place in wants under each cap set, in CAP_SETS' order
    for call in CALLS:
        for cap_name, (caps, moment) in CAP_SETS.items():
            want = ""
            for state, fl in rows(call, cap_name):
                quiet = dict(field_differs=0, pred_usable=0, eh_current=0, modes_current=0, optimize_due_any=0, output_follows=0)
                refusal, after, pair, nxt, acts = answer(call, state, dict(moment, **dict(quiet, **fl)), caps)
                # "<refusal, one character of ALPHABET><refused after: 0 | 1><the state that follows, STATE's fields in order: a digit
                # each, . where the field keeps the value it came with>[!<the refused pair: seq, owed>] <the action list>"; an action
                # list: "<index in acts>[:<argument>] ..."
                bad = "" if refusal != "IllegalState" else "!%d%d" % (SEQ.index(pair[0]), OWED.index(pair[1]))
                came = [SEQ.index(state["seq"]), OWED.index(state["owed"])] + [int(state[n]) for n in STATE[2:]]
                goes = [SEQ.index(nxt[0]), OWED.index(nxt[1])] + [int(v) for v in nxt[2:]]
                i = answers("%s%d%s%s %d" % (ALPHABET[REFUSALS.index(refusal)], after, "".join("." if c == g else str(g) for c, g in zip(came, goes)),
                                            bad, act_lists(" ".join(str(ACTS.index(n)) if not a else "%d:%d" % (ACTS.index(n), a) for n, a in acts))))
                want += ALPHABET[i // len(ALPHABET)] + ALPHABET[i % len(ALPHABET)]
                nrows += 1
            groups.setdefault(call, []).append(wants(want))
    assert len(answers.items) <= len(ALPHABET) ** 2
    table = dict(seq=SEQ, owed=OWED, state=STATE, refusals=REFUSALS, acts=ACTS, pairs=PAIRS, variants=VARIANTS, variants_under=VARIANTS_UNDER, flags=FLAGS,
                 cap_sets={n: dict(caps=c, moment=m) for n, (c, m) in CAP_SETS.items()}, alphabet=ALPHABET, act_lists=act_lists.items,
                 answers=answers.items, wants=wants.items, groups=groups)
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in table.items()) + "\n}\n")
    print(out, sum(len(g) for g in groups.values()), "groups,", nrows, "rows,", len(answers.items), "distinct answers,", len(act_lists.items), "action lists,",
          len(wants.items), "distinct groups")
