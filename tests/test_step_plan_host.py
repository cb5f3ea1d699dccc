"""What a time step launches (pic1dp_amd/csrc/step_plan.cpp: step_caps, plan_markers, plan_solve, plan_whole_step) against a
table transcribed from the conditions as capi_step.cpp held them before they became pure functions
(tests/golden/gen_step_plan.py), through the probe library.  No GPU."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUT_KEYS = ("nx", "nm", "ns", "nparticle_max", "iptcldist", "deltaf", "linear", "nx_opd", "nv_opd", "layout", "np", "pow2", "one_exp")


@pytest.fixture(scope="module")
def probe():
    from pic1dp_amd import probe as p
    p.load()
    return p


@pytest.fixture(scope="module")
def table():
    """the recorded table: per group the axes (every combination is a row, in order; an axis of dicts sets several fields) and
    the answers' recorded sections"""
    import itertools
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "step_plan.json")))
    t["rows"] = []
    for g in t["groups"]:
        combos = list(itertools.product(*g["axes"].values()))
        assert len(combos) == len(g["want"])
        for combo, want in zip(combos, g["want"]):
            given = dict(g["fixed"])
            for name, v in zip(g["axes"], combo):
                given.update(v if isinstance(v, dict) else {name: v})
            t["rows"].append(dict(group=g["name"], sections=g["sections"], query=dict(t["base"], **given), given=given, want=want))
    return t


def ask(probe, q, sections):
    """the library's answer to a full query, its sections flattened as the table stores them"""
    import pic1dp_amd
    ns, nm = q["ns"], q["nm"]
    inp = pic1dp_amd.make_input(nx=q["nx"], nmode=nm, modes=list(range(1, nm + 1)), nspecies=ns, nparticle_max=q["nparticle_max"],
                                species_charge=[-1.0, 1.0][:ns], species_mass=[1.0, 2.0][:ns], iptcldist=q["iptcldist"],
                                deltaf=q["deltaf"], linear=q["linear"], nx_opd=q["nx_opd"], nv_opd=q["nv_opd"])
    nranks, npe, rank = q["layout"]
    a = probe.host_step_plan(inp, nranks=nranks, npe=npe, rank=rank, np_=q["np"], pow2=q["pow2"], one_exp=q["one_exp"],
                             **{k: v for k, v in q.items() if k not in INPUT_KEYS})
    sp = a["markers"]["species"]
    part = {"caps": list(a["caps"].values()), "solve": list(a["solve"].values()), "whole": list(a["whole"].values()),
            "carry": [L["carry"] for L in sp],
            "markers": [a["markers"][n] for n in probe.STEP_MARKERS] + [L[n] for L in sp for n in probe.STEP_SPECIES]}
    return sum((part[sec] for sec in sections), []) + ([L["name"] for L in sp] if "markers" in sections else [])


def fields(probe, sections, ns):
    part = {"caps": ["caps." + n for n in probe.STEP_CAPS], "solve": ["solve." + n for n in probe.STEP_SOLVE],
            "whole": ["whole." + n for n in probe.STEP_WHOLE], "carry": ["species%d.carry" % s for s in range(ns)],
            "markers": ["markers." + n for n in probe.STEP_MARKERS] + ["species%d.%s" % (s, n) for s in range(ns) for n in probe.STEP_SPECIES]}
    return sum((part[sec] for sec in sections), []) + (["species%d.name" % s for s in range(ns)] if "markers" in sections else [])


def test_every_plan_is_the_recorded_one(probe, table):
    """row by row, every field of the sections the row's group records; each of the four results is recorded whole by several groups"""
    assert {sec for g in table["groups"] for sec in g["sections"]} == {"caps", "markers", "solve", "whole", "carry"}
    bad = []
    for row in table["rows"]:
        got = ask(probe, row["query"], row["sections"])
        names = fields(probe, row["sections"], row["query"]["ns"])
        assert len(got) == len(row["want"]) == len(names)
        diff = {n: (g, w) for n, g, w in zip(names, got, row["want"]) if g != w}
        if diff:
            bad.append((row["group"], row["given"], diff))
    assert not bad, "%d rows differ; (got, recorded) of the first: %r" % (len(bad), bad[:3])


def test_the_table_sits_on_the_turning_points(probe, table):
    """a row on each side of every threshold, and the recorded answer changes between them"""
    def rows(group, **given):
        out = [dict(zip(fields(probe, r["sections"], r["query"]["ns"]), r["want"]), **{"q." + k: v for k, v in r["query"].items()})
               for r in table["rows"] if r["group"] == group and all(r["query"][k] == v for k, v in given.items())]
        assert out, (group, given)
        return out

    def one(group, field, **given):
        vals = {r[field] for r in rows(group, **given)}
        assert len(vals) == 1, (group, field, given, vals)
        return vals.pop()

    t = table["turning"]
    # LDS limits: the whole-step kernels' tiles against the cap, kind 0 and 1 of the charge sum
    for cs, nx in ((0, t["nx_step"]), (1, t["nx_step_exact"])):
        assert one("step_lds", "caps.step_recompute_ok", nx=nx, charge_sum=cs) == 1
        assert one("step_lds", "caps.step_recompute_ok", nx=nx + 1, charge_sum=cs) == 0
        assert one("step_lds", "whole.substeps", nx=nx + 1, charge_sum=cs) == 1
    assert t["nx_step_exact"] < t["nx_step"]
    # the diagnostics' LDS need, nx_opd 0 | 1, nv_opd 1 | 2
    assert one("diag_lds", "markers.diag", nx_opd=1, nv_opd=2, full=1) == 1 and one("diag_lds", "markers.diag", nx_opd=0, nv_opd=2, full=1) == 0
    assert one("diag_lds", "markers.diag", nx_opd=1, nv_opd=1, full=1) == 0 and one("diag_lds", "markers.diag", nx_opd=1, nv_opd=2, full=0) == 0
    assert one("diag_lds", "markers.diag", nx_opd=t["nxo_diag"], nv_opd=64, full=1) == 1
    assert one("diag_lds", "markers.diag", nx_opd=t["nxo_diag"] + 1, nv_opd=64, full=1) == 0
    assert one("diag_lds", "species0.name", nx_opd=1, nv_opd=2, full=1) == "k_step_full<DIAG>"
    # a launch that can carry the solve, and launches that cannot: one wave; an oversubscribed grid
    assert one("fused_fit", "caps.fuse_capable", threads_req=0, nparticle_max=1001, nx=32) == 1
    assert one("fused_fit", "markers.solve_fits", threads_req=64, nparticle_max=1001, nx=32) == 0
    assert one("fused_fit", "caps.fuse_capable", threads_req=64, nparticle_max=1001, nx=32) == 0
    assert one("fused_fit", "caps.fuse_capable", threads_req=128, nparticle_max=1001, nx=32) == 1
    assert one("fused_fit", "caps.fuse_capable", threads_req=0, nparticle_max=100000001, nx=32) == 0
    # kept modes against the one-workgroup field kernels
    assert one("modes_fit", "caps.modes_fit_field_kernel", nm=128) == 1 and one("modes_fit", "caps.modes_fit_field_kernel", nm=129) == 0
    assert one("modes_fit", "solve.launch", nm=128, pred_fresh=1, layout=[1, 0, 0], comm=0) == 2
    assert one("modes_fit", "solve.launch", nm=129, pred_fresh=1, layout=[1, 0, 0], comm=0) == 0
    assert one("modes_fit", "solve.pack_reduce", nm=128, pred_fresh=1, layout=[2, 2, 0], comm=1) == 1
    assert one("modes_fit", "solve.pack_reduce", nm=129, pred_fresh=1, layout=[2, 2, 0], comm=1) == 0
    # which one-pass kernel: none, tiles, sums in registers, private sums; a thread count by hand takes the private sums away
    seen = {(r["caps.pred_kind"], r["caps.priv"], r["q.threads_req"]) for r in rows("pred_kind")}
    assert seen == {(k, p, th) for k, p in ((0, 0), (1, 0), (2, 0), (2, 1)) for th in (0, 64)} - {(2, 1, 64)}
    assert {r["species0.name"] for r in rows("pred_kind")} == {"k_step_full", "k_step_one", "k_step_sums", "k_step_one<sums>"}
    assert one("eh_modes", "markers.pred", pred_kind_req=3, eh_modes=0) == 0 and one("eh_modes", "markers.pred", pred_kind_req=3, eh_modes=1) == 1
    assert one("eh_modes", "markers.pred", pred_kind_req=0, eh_modes=0) == 1      # (the private sums stage Eh from its tile)
    # the fused solve against the chain's length: 1024 | 1025 terms without the matrix unit, with it, and by npe
    for mfma, nx in ((0, 1024), (1, 3074)):
        assert one("fuse_chain", "caps.fuse_capable", fuse_solve=1, nx=nx, chain_mfma=mfma) == 1
        assert one("fuse_chain", "caps.fuse_capable", fuse_solve=1, nx=nx + 1, chain_mfma=mfma) == 0
        assert one("fuse_chain", "caps.fuse_capable", fuse_solve=2, nx=nx + 1, chain_mfma=mfma) == 1
        assert one("fuse_chain", "caps.fuse_capable", fuse_solve=0, nx=nx, chain_mfma=mfma) == 0
    assert one("fuse_npe", "caps.fuse_capable", fuse_solve=2, field_npe=32, nx=32) == 1 and one("fuse_npe", "caps.fuse_capable", fuse_solve=2, field_npe=33, nx=32) == 0
    assert one("fuse_npe", "caps.fuse_capable", fuse_solve=1, field_npe=1, nx=1025) == 0 and one("fuse_npe", "caps.fuse_capable", fuse_solve=1, field_npe=32, nx=1025) == 1
    # fused in and out against the moment
    m = dict(optimize_now=0, fuse_output=0)
    assert one("moment", "whole.fused_in", pending=1, **m) == 1 and one("moment", "whole.finish_pending", pending=1, **m) == 0
    assert one("moment", "whole.fuse_out", steps_left=1, **m) == 0 and one("moment", "whole.fuse_out", steps_left=2, optimize_next=0, **m) == 1
    assert one("moment", "whole.fuse_out", steps_left=3, optimize_next=1, **m) == 0
    assert one("moment", "whole.fuse_out", steps_left=2, output_next=1, optimize_next=0, optimize_now=0, fuse_output=2) == 0
    assert one("moment", "whole.fuse_out", steps_left=3, output_next=1, optimize_next=0, optimize_now=0, fuse_output=2) == 1
    assert one("moment", "whole.substeps", optimize_now=1) == 1 and one("moment", "whole.finish_pending", optimize_now=1, pending=1) == 1
    assert one("moment", "whole.fused_in", pending=1, steps_left=1, output_now=1, optimize_now=0, fuse_output=2) == 0
    assert one("moment", "whole.finish_pending", pending=1, steps_left=1, output_now=1, optimize_now=0, fuse_output=2) == 1
    assert one("moment_no_fuse", "whole.finish_pending", pending=1) == 1
    assert one("moment_no_fuse", "whole.half_pass", pending=0, have_eh=0) == 1 and one("moment_no_fuse", "whole.half_pass", predict=0) == 1
    assert one("moment_no_fuse", "whole.adopt_eh", have_eh=1, predict=1) == 1 and one("moment_no_fuse", "whole.adopt_eh", have_eh=1, predict=0) == 0
    # output fusion against predict_capable; the exact sums keep the diagnostics' own pass
    f = dict(diag_sum=0, charge_sum=0)
    assert [one("fuse_output", "whole.diag", fuse_output=o, predict=1, **f) for o in (0, 1, 2)] == [0, 0, 1]
    assert [one("fuse_output", "whole.diag", fuse_output=o, predict=0, **f) for o in (0, 1, 2)] == [0, 1, 1]
    assert one("fuse_output", "whole.diag", diag_sum=1) == 0 and one("fuse_output", "whole.diag", charge_sum=1) == 0
    # carry: every combination is there; the default carries only without the one-exp form
    assert len(rows("carry")) == 4 * 4 * 2 * 2 * 3 * 3
    assert {r["species0.carry"] for r in rows("carry")} == {0, 1, 2}
    c = dict(deltaf=1, linear=0, pow2=[0, 0])
    assert one("carry", "species0.carry", carry=-1, iptcldist=3, one_exp=[0, 0], pred=0, full=1, **c) == 1
    assert one("carry", "species0.carry", carry=-1, iptcldist=3, one_exp=[1, 0], pred=0, full=1, **c) == 0
    assert one("carry", "species0.carry", carry=-1, iptcldist=2, one_exp=[0, 0], pred=0, full=1, **c) == 0
    assert one("carry", "species0.carry", carry=2, iptcldist=2, one_exp=[0, 0], pred=0, full=1, **c) == 1
    assert one("carry", "species0.carry", carry=-1, iptcldist=2, one_exp=[0, 0], pred=1, full=1, **c) == 2
    assert one("carry", "species0.carry", carry=-1, iptcldist=2, one_exp=[1, 0], pred=1, full=1, **c) == 0
    assert one("carry", "species0.carry", carry=1, iptcldist=2, one_exp=[1, 0], pred=1, full=1, **c) == 2
    assert one("carry", "species0.carry", carry=0) == 0 and one("carry", "species0.carry", deltaf=0) == 0
    # the other solver and the other transform: none of the fused or predicted paths
    for other in (dict(field_solver=1), dict(field_transform=1)):
        assert one("field_paths", "caps.dft_paths", **other) == 0 and one("field_paths", "caps.predict_capable", **other) == 0
        assert one("field_paths", "solve.launch", **other) == 0 and one("field_paths", "whole.fused_in", **other) == 0
    assert one("field_paths", "solve.launch", field_solver=0, field_transform=0, pred_fresh=1) == 2
    # streaming: both thresholds, and the override
    assert t["nt_full"] == 9437184
    assert one("streaming", "markers.stream_nt", nparticle_max=t["nt_full"], full=1) == 0 and one("streaming", "markers.stream_nt", nparticle_max=t["nt_full"] + 1, full=1) == 1
    assert one("streaming", "markers.stream_nt", nparticle_max=t["nt_half"], full=0) == 0 and one("streaming", "markers.stream_nt", nparticle_max=t["nt_half"] + 1, full=0) == 1
    assert one("streaming", "species0.plain_chunks", nparticle_max=t["nt_full"], full=1, pred=1) == 0
    assert one("streaming", "species0.plain_chunks", nparticle_max=t["nt_full"] + 1, full=1, pred=1) == 65536
    assert one("streaming", "species0.plain_chunks", nparticle_max=t["nt_full"] + 1, full=1, pred=0) == 0
    assert [one("nt_force", "markers.stream_nt", nt_force=f, full=1, nparticle_max=1001) for f in (-1, 0, 1, 2, 3)] == [0, 0, 1, 0, 1]
    assert [one("nt_force", "markers.stream_nt", nt_force=f, full=0, nparticle_max=t["nt_full"] + 1) for f in (-1, 0, 1, 2, 3)] == [0, 0, 1, 1, 0]
    # the tail: one rank never, a communicator packs, the exchange posts; PIC1DP_TAIL=0, the tiles and a sub-step: none
    tl = dict(tail_on=1, tail_ok=1, pred_kind_req=0)
    assert one("tail", "markers.tail_mode", layout=[1, 0, 0], comm=0, xchg=0, **tl) == 0
    assert one("tail", "markers.tail_mode", layout=[1, 0, 0], comm=1, **tl) == 1 and one("tail", "markers.tail_mode", layout=[2, 2, 0], comm=1, **tl) == 1
    assert one("tail", "markers.tail_mode", layout=[2, 2, 0], xchg=1, **tl) == 2 and one("tail", "markers.tail_mode", layout=[2, 2, 0], comm=0, xchg=0, **tl) == 0
    assert one("tail", "markers.tail_mode", tail_on=0) == 0 and one("tail", "markers.tail_mode", tail_ok=0) == 0 and one("tail", "markers.tail_mode", pred_kind_req=1) == 0
    # every combination of prediction x ranks x target x tail, the two refused ones included
    assert len(rows("solve")) == 2 * 5 * 2 * 3 * 2
    assert {r["solve.refused"] for r in rows("solve")} == {0, 1, 2} and {r["solve.launch"] for r in rows("solve", charge_sum=0)} == {0, 1, 2, 3, 4, 5}
    s = dict(charge_sum=0, pred_fresh=1, into_E=1)
    assert one("solve", "solve.launch", layout=[2, 2, 0], comm=1, tail_done=1, **s) == 3 and one("solve", "solve.pack_first", layout=[2, 2, 0], comm=1, tail_done=1, **s) == 0
    assert one("solve", "solve.pack_first", layout=[2, 2, 0], comm=1, tail_done=0, **s) == 1
    assert one("solve", "solve.launch", layout=[2, 2, 0], xchg=1, tail_done=2, **s) == 5 and one("solve", "solve.launch", layout=[2, 2, 0], xchg=1, tail_done=0, **s) == 4
    assert one("solve", "solve.refused", layout=[1, 0, 0], comm=0, tail_done=1, **s) == 1 and one("solve", "solve.refused", layout=[2, 2, 0], xchg=1, tail_done=2, charge_sum=0, pred_fresh=0) == 2
    assert one("solve", "solve.reduce_first", layout=[2, 2, 0], comm=0, xchg=0, tail_done=0, charge_sum=0) == 1
    assert one("solve", "solve.reduce_first", charge_sum=1, tail_done=0) == 0 and one("solve", "solve.with_local", charge_sum=1, tail_done=0) == 1
    # two species, the first one empty: the second carries the solve and the tail
    e = dict(np=[0, 1001], pred=1)
    assert one("species", "species0.launched", **e) == 0 and one("species", "markers.solve_species", **e) == 1
    assert one("species", "markers.tail_species", layout=[2, 2, 0], **e) == 1 and one("species", "species1.tail", layout=[2, 2, 0], **e) == 1
    assert one("species", "markers.solve_species", np=[0, 0], pred=1) == -1 and one("species", "caps.fuse_capable", np=[0, 0], layout=[1, 0, 0]) == 0
    assert one("species", "species1.name", np=[1001, 501], pred=1, one_exp=[0, 1]) == "k_step_one<sums> (one-exp -f0'/f0)"


def test_the_probe_refuses_what_it_cannot_answer(probe):
    import pic1dp_amd
    inp = pic1dp_amd.make_input(nx=32, nparticle_max=1001)
    with pytest.raises(ValueError):
        probe.host_step_plan(inp, nranks=0)
