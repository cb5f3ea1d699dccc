"""tests/golden/step_plan.json: what a time step launches, transcribed from the conditions as they stood in capi_step.cpp
(cited below as :line, at the commit before step_plan.cpp took them over) with the launch shapes of launch_policy.cpp and
the context's plan of gen_context_plan.py.  Nothing here calls the library.  Run once; tests/test_step_plan_host.py reads
the table.
    python tests/golden/gen_step_plan.py"""
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_context_plan as gcp  # noqa: E402

PARTICLE_LDS_CAP, CU_LDS, STATIC_LDS = gcp.PARTICLE_LDS_CAP, gcp.CU_LDS, gcp.STATIC_LDS
FIELD_THREADS, PRIV_THREADS = 256, gcp.PRIV_THREADS
TAG_HALF, TAG_FULL, TAG_ONE = 103, 104, 106          # timing.hpp
PLAIN_STATE_BYTES = 256 << 20                        # launch_policy.hpp kPlainStateBytes
even = gcp.even

# a query: the input, the layout, and the fields of pic1dp_probe_step_query (include/pic1dp_probe.h)
BASE = dict(nx=32, nm=1, ns=1, nparticle_max=1001, np=None, iptcldist=3, deltaf=1, linear=0, nx_opd=16, nv_opd=32, layout=[1, 0, 0],
            fuse_solve=1, tail_on=1, call_pair=1, lazy_calls=1, predict=1, carry=-1, osub_req=0, dyn_tail=8, dyn_tail_full=16,
            pred_kind_req=0, nt_threshold_half=2048.0 * 1048576.0, nt_threshold_full=288.0 * 1048576.0, num_cu=256, threads_req=0,
            bpc_req=0, charge_sum=0, diag_sum=0, fuse_output=0, step_mode=0, field_solver=0, field_transform=0, comm=0, xchg=0,
            field_npe=0, chain_mfma=0, has_pred=-1, pow2=[0, 0], one_exp=[0, 0], full=1, diag=0, pred=1, tail_ok=1, eh_modes=2,
            nt_force=-1, pred_fresh=1, tail_done=0, into_E=1, pending=0, have_eh=1, steps_left=3, output_now=0, output_next=0,
            optimize_now=0, optimize_next=0)


# ---- kernels.hpp: dynamic LDS of the whole-step kernels ----
def step_lds_bytes(nx, full, exact=False):
    return 8 * ((2 if full else 1) * even(nx) + (2 if exact else 1) * even(nx) + 2)


def step_diag_lds_bytes(nxo, nvo):
    return 8 * (3 * nxo * nvo + 3 * nvo + 16)


# ---- launch_policy.cpp ----
NEVER, IF_ASKED, AUTO = 0, 1, 2


def oversubscribed(q, nx, np_, resident, how):
    if how == NEVER or q["bpc_req"] > 0:
        return resident
    f = q["osub_req"]
    if f <= 0 and how != AUTO:
        return resident
    if f <= 0:
        f = (np_ // (48 * nx) + resident // 2) // max(resident, 1)
    return resident * max(1, min(f, 64 if q["osub_req"] > 0 else 4))


def grid_of(q, nx, np_, threads, bpc, how):
    resident = q["num_cu"] * bpc
    need = ((np_ >> 1) + threads - 1) // threads
    return resident, max(1, min(oversubscribed(q, nx, np_, resident, how), need))


def workgroups_per_cu(q, bpc, by_lds):
    bpc = min(bpc, by_lds)
    if q["bpc_req"] > 0:
        bpc = min(q["bpc_req"], by_lds)
    return max(bpc, 1)


def step_launch(q, nx, np_, full, exact):
    lds = step_lds_bytes(nx, full, exact)
    by_lds = max(1, CU_LDS // (lds + STATIC_LDS))
    req = q["threads_req"]
    threads = req if req > 0 else (1024 if by_lds < 2 else 768)
    bpc = workgroups_per_cu(q, 2048 // threads if req > 0 else (2 if threads == 768 else 1), by_lds)
    return threads, grid_of(q, nx, np_, threads, bpc, AUTO if not full and bpc >= 2 else IF_ASKED)[1], lds


def step_diag_launch(q, nx, np_, exact, nxo, nvo):
    return 1024, grid_of(q, nx, np_, 1024, 1, NEVER)[1], step_lds_bytes(nx, True, exact) + step_diag_lds_bytes(nxo, nvo)


def pred_launch(q, nx, nm, np_, priv, kind, exp_bearing):
    lds = gcp.step_one_private_lds_bytes(nx) if priv else (gcp.step_sums_lds_bytes(nx) if kind == 2 else gcp.step_one_lds_bytes(nx, nm))
    two = 2 * (lds + STATIC_LDS) <= CU_LDS
    th2, th1 = 768, 1024
    if priv:
        th2 = th1 = PRIV_THREADS
    if kind == 2 and not priv:
        if exp_bearing:
            two = False
        else:
            th1 = 512
    threads = q["threads_req"] if q["threads_req"] > 0 else (th2 if two else th1)
    bpc = q["bpc_req"] if q["bpc_req"] > 0 else (2 if two else 1)
    resident, blocks = grid_of(q, nx, np_, threads, bpc, AUTO if bpc >= 2 else IF_ASKED)
    return (threads, blocks, lds), resident


def fits_fused_solve(shape, resident):     # launch_policy.hpp
    return shape[1] <= resident and shape[0] >= 128 and shape[0] % 64 == 0


def stream_plain_chunks(np_all, np_s, nt):
    if not nt or np_s <= 0 or np_all < np_s:
        return 0
    return min(int(float(np_s) / float(np_all) * float(PLAIN_STATE_BYTES)) // 4096, ((np_s >> 1) + 63) >> 6)


# ---- the context: plan_context as gen_context_plan.py transcribes it ----
def context(q):
    gcp.NPARTICLE_MAX = q["nparticle_max"]
    gcp.NPARTICLE_INIT = [q["nparticle_max"]] * 2
    p = gcp.plan(q["nx"], q["nm"], q["ns"], pred_req=q["pred_kind_req"], layout=tuple(q["layout"]))
    np_ = [p["np"][s] if q["np"] is None or q["np"][s] < 0 else q["np"][s] for s in range(q["ns"])]
    several = q["layout"][0] > 1 or q["comm"] != 0                                     # ctx.hpp several_ranks
    return dict(kind=p["pred_kind"], private=p["pred_private"], npe=q["field_npe"] or p["field_npe"], np=np_, several=several,
                has_pred=p["pred_kind"] != 0 if q["has_pred"] < 0 else q["has_pred"] != 0)


# ---- capi_step.cpp as it was ----
def caps(q, c):
    k = {}
    k["dft_paths"] = q["field_solver"] == 0 and q["field_transform"] == 0                                # :17
    k["six_sums_one_mode"] = c["kind"] == 2 and q["nm"] == 1                                             # :20
    k["modes_fit_field_kernel"] = 2 * q["nm"] <= FIELD_THREADS                                           # :22
    k["exp_bearing"] = bool(q["deltaf"]) and q["iptcldist"] in (2, 3)                                    # :24
    k["step_recompute_ok"] = q["step_mode"] == 0 and step_lds_bytes(q["nx"], True, q["charge_sum"] == 1) <= PARTICLE_LDS_CAP  # :40-42
    k["predict_capable"] = (q["charge_sum"] == 0 and bool(q["predict"]) and c["kind"] != 0 and c["has_pred"] and k["dft_paths"]
                            and k["step_recompute_ok"])                                                  # :57-59
    k["diag_in_step"] = q["charge_sum"] == 0 and q["diag_sum"] == 0 and (
        q["fuse_output"] == 2 or (q["fuse_output"] == 1 and not k["predict_capable"]))                    # :68-70
    k["priv"] = c["kind"] == 2 and bool(c["private"]) and q["threads_req"] <= 0                          # :233
    # fuse_capable :100-115, fused_solve_launch_fits :83-91 (priv there: plan.pred_private && threads_req <= 0 -- under
    # six_sums_one_mode the same thing)
    fuse = bool(q["fuse_solve"]) and not c["several"] and k["six_sums_one_mode"] and k["dft_paths"] and c["npe"] <= 32 and k["predict_capable"]
    if fuse:
        chain_terms = q["nx"] // 3 if (c["npe"] == 1 and q["chain_mfma"]) else q["nx"] // max(1, c["npe"])
        if q["fuse_solve"] != 2 and chain_terms > 1024:
            fuse = False
    if fuse:
        first = [n for n in c["np"] if n > 0]
        fuse = bool(first) and fits_fused_solve(*pred_launch(q, q["nx"], q["nm"], first[0], bool(c["private"]) and q["threads_req"] <= 0,
                                                             c["kind"], k["exp_bearing"]))
    k["fuse_capable"] = fuse
    k["lazy_calls_ok"] = bool(q["lazy_calls"]) and k["step_recompute_ok"]                                # lazy_ok :840-842, without the event
    k["pair_serves_collect"] = (bool(q["call_pair"]) and bool(q["lazy_calls"]) and not c["several"] and k["predict_capable"]
                                and k["six_sums_one_mode"])                                              # collect_charge :954-955
    k["pair_in_solve_field"] = (bool(q["call_pair"]) and bool(q["lazy_calls"]) and k["dft_paths"] and k["predict_capable"]
                                and k["six_sums_one_mode"])                                              # solve_field :1054-1055 (pred_usable :119-122)
    k["pred_kind"] = c["kind"]
    return {n: int(v) for n, v in k.items()}


def markers(q, c, k):
    nx, ns, full, exact = q["nx"], q["ns"], bool(q["full"]), q["charge_sum"] == 1
    pred, diag = bool(q["pred"]), bool(q["diag"])
    if pred and (not full or diag or not k["predict_capable"]):                                          # plan_step :232
        pred = False
    priv = bool(k["priv"])                                                                               # :233
    if pred and c["kind"] == 2 and not priv and q["eh_modes"] == 0:                                      # :234
        pred = False
    if diag:                                                                                             # :238-242
        need = step_lds_bytes(nx, True) + step_diag_lds_bytes(q["nx_opd"], q["nv_opd"])
        if not full or q["nx_opd"] < 1 or q["nv_opd"] < 2 or need > PARTICLE_LDS_CAP:
            diag = False
    tail_mode, tail_species = 0, -1                                                                      # :246-252
    if q["tail_ok"] and pred and q["tail_on"] and k["six_sums_one_mode"] and k["dft_paths"] and c["several"]:
        tail_mode = 2 if q["xchg"] else (1 if q["comm"] else 0)
        for s in range(ns):
            if c["np"][s] > 0:
                tail_species = s
        if tail_species < 0:
            tail_mode = 0
    state_bytes = sum(32.0 * n for n in c["np"])                                                         # :254-256
    nt = int(state_bytes > (q["nt_threshold_full"] if full else q["nt_threshold_half"]))
    f = q["nt_force"]                                                                                    # :257-263
    nt = {0: 0, 1: 1, 2: 0 if full else 1, 3: 1 if full else 0}.get(f, nt)
    m = dict(pred=int(pred), priv=int(priv), diag=int(diag), tail_mode=tail_mode, tail_species=tail_species, stream_nt=nt,
             solve_species=-1, solve_fits=0, solve_threads=0, tag=TAG_ONE if pred else (TAG_FULL if full else TAG_HALF),       # :403
             rd=8 * (3 + (1 if q["deltaf"] else 0)),                                                                            # :406
             wr=8 * (1 + (0 if q["linear"] else 1) + (1 if q["deltaf"] else 0)) if full else 0, species=[])                      # :407
    for s in range(ns):
        n = c["np"][s]
        L = dict(launched=0, family=0, threads=0, blocks=0, lds=0, dyn_tail=0, plain_chunks=0, carry=0, tail=0, name="")
        m["species"].append(L)
        if n <= 0:                                                                                       # step_particles :436
            continue
        L["launched"] = 1
        L["dyn_tail"] = q["dyn_tail_full"] if full and not pred else q["dyn_tail"]                        # :369
        L["threads"], L["blocks"], L["lds"] = step_launch(q, nx, n, full, exact)                         # :371
        if not pred:                                                                                     # wire_carry :283-284
            if (q["carry"] != 0 and q["deltaf"] and not q["pow2"][s] and not q["one_exp"][s]
                    and (q["iptcldist"] == 3 or (q["carry"] == 2 and q["iptcldist"] == 2))):
                L["carry"] = 1
        else:                                                                                            # :299-300 (kCarryOneExpDefault false)
            carry_one = (not q["one_exp"][s]) if q["carry"] < 0 else q["carry"] > 0
            if k["exp_bearing"] and carry_one:
                L["carry"] = 2
            L["family"] = (2 if priv else 1) if c["kind"] == 2 else 0                                    # :387
            shape, resident = pred_launch(q, nx, q["nm"], n, priv, c["kind"], bool(k["exp_bearing"]))    # :393
            L["threads"], L["blocks"], L["lds"] = shape
            L["plain_chunks"] = stream_plain_chunks(sum(c["np"]), n, nt != 0)                            # :394-398
            if m["solve_species"] < 0:                                                                   # :372-379: the first species launched
                m["solve_species"], m["solve_fits"], m["solve_threads"] = s, int(fits_fused_solve(shape, resident)), shape[0]
            L["tail"] = int(tail_mode != 0 and s == tail_species)                                        # :399
        if diag:                                                                                         # wire_diag :336
            L["threads"], L["blocks"], L["lds"] = step_diag_launch(q, nx, n, exact, q["nx_opd"], q["nv_opd"])
        base = (("k_step_one<sums>" if priv else "k_step_sums") if c["kind"] == 2 else "k_step_one") if pred else (
            ("k_step_full<DIAG>" if diag else "k_step_full") if full else "k_step_half")                 # :410-412
        L["name"] = base + ("<EXACT>" if exact else "") + (" (one-exp -f0'/f0)" if q["one_exp"][s] and q["deltaf"] else "")
    return m


def solve(q, c, k):                                                                                      # solve_phase :526-597
    fresh, into_E, tail_done = bool(q["pred_fresh"]), bool(q["into_E"]), q["tail_done"]
    multi = q["charge_sum"] == 0 and c["several"]                                                        # :529 fp64_rank_sum
    fused_xchg = multi and bool(q["xchg"]) and bool(k["dft_paths"])                                      # :530
    will_pack = (fresh and multi and not fused_xchg and bool(q["comm"]) and not q["xchg"] and bool(k["dft_paths"])
                 and bool(k["modes_fit_field_kernel"]) and into_E)                                       # :532-533
    out = dict(refused=0, reduce_first=0, pack_reduce=0, pack_first=0, launch=0, with_local=0)
    if tail_done == 1 and not will_pack:                                                                 # :536
        return dict(out, refused=1)
    if tail_done == 2 and not (fused_xchg and fresh):                                                    # :537-538
        return dict(out, refused=2)
    out["pack_reduce"] = int(will_pack)                                                                  # :539
    out["pack_first"] = int(will_pack and tail_done != 1)                                                # :540
    out["reduce_first"] = int(not will_pack and multi and not fused_xchg)                                # :549
    out["with_local"] = int(not multi)                                                                   # :592
    pair = (fresh and (not multi or fused_xchg or will_pack) and bool(k["dft_paths"]) and bool(k["modes_fit_field_kernel"])
            and into_E)                                                                                  # :565-566
    if pair:                                                                                             # :574-585
        out["launch"] = 3 if will_pack else ((5 if tail_done == 2 else 4) if fused_xchg else 2)
    else:                                                                                                # :590-592
        out["launch"] = 1 if fused_xchg else 0
    return out


def whole(q, k):                                                                                         # pic1dp_hip_step :683-733
    w = dict(substeps=0, finish_pending=0, diag=0, pred=0, fused_in=0, adopt_eh=0, half_pass=0, half_eh_modes=0, fuse_out=0)
    pending = bool(q["pending"])
    if not (k["step_recompute_ok"] and not q["optimize_now"]):                                           # :686, :722-726
        return dict(w, substeps=1, finish_pending=int(pending))
    pc = bool(k["predict_capable"])                                                                      # :690
    diag = bool(k["diag_in_step"]) and q["steps_left"] == 1 and bool(q["output_now"])                    # :692
    pred = pc and not diag                                                                               # :693
    fused_in = pending and pred and bool(k["fuse_capable"])                                              # :695
    have_eh = pc and bool(q["have_eh"])                                                                  # :699
    fuse_out = False
    if pred and q["steps_left"] > 1 and k["fuse_capable"]:                                               # :712-717
        next_diag = bool(k["diag_in_step"]) and q["steps_left"] == 2 and bool(q["output_next"])
        fuse_out = not next_diag and not q["optimize_next"]
    return dict(w, finish_pending=int(pending and not fused_in), diag=int(diag), pred=int(pred), fused_in=int(fused_in),
                adopt_eh=int(not fused_in and have_eh), half_pass=int(not fused_in and not have_eh),
                half_eh_modes=int(k["dft_paths"]), fuse_out=int(fuse_out))                               # :696-708


def answer(query):
    q = dict(BASE, **query)
    c = context(q)
    k = caps(q, c)
    return dict(caps=k, markers=markers(q, c, k), solve=solve(q, c, k), whole=whole(q, k))


def last_fit(fits):
    nx = 8
    while fits(nx + 1):
        nx += 1
    return nx


NX_STEP = last_fit(lambda nx: step_lds_bytes(nx, True, False) <= PARTICLE_LDS_CAP)       # kind 0 of the charge sum
NX_STEP_EXACT = last_fit(lambda nx: step_lds_bytes(nx, True, True) <= PARTICLE_LDS_CAP)  # kind 1
NXO_DIAG = last_fit(lambda a: step_lds_bytes(32, True) + step_diag_lds_bytes(a, 64) <= PARTICLE_LDS_CAP)   # nx 32, nv_opd 64
NT_FULL, NT_HALF = 288 * 1048576 // 32, 2048 * 1048576 // 32                             # markers at the two thresholds
RANKS = [dict(), dict(comm=1), dict(layout=[2, 2, 0], comm=1), dict(layout=[2, 2, 0], xchg=1), dict(layout=[2, 2, 0])]
PHYSICS = [dict(deltaf=1, linear=0), dict(deltaf=1, linear=1), dict(deltaf=0, linear=0)]
LAUNCHES = [dict(pred=1, full=1), dict(pred=0, full=1), dict(pred=0, full=0)]

# (group, what it records of the answer, the queries' common part, the axes: every combination in this order is a row; an
# axis whose values are dicts sets several fields at once).  "carry": the species' carry decisions alone.
GROUPS = [
    # LDS limits and launch fit
    ("step_lds", ["caps", "whole"], dict(nparticle_max=200001),
     dict(nx=[NX_STEP, NX_STEP + 1, NX_STEP_EXACT, NX_STEP_EXACT + 1], charge_sum=[0, 1])),
    ("diag_lds", ["markers"], dict(diag=1, fuse_output=2, pred=0), dict(nx_opd=[0, 1, NXO_DIAG, NXO_DIAG + 1], nv_opd=[1, 2, 64], full=[0, 1])),
    ("fused_fit", ["caps", "markers"], {}, dict(threads_req=[0, 64, 128], nparticle_max=[1001, 100000001])),
    # modes and prediction kind
    ("modes_fit", ["caps", "solve"], dict(nx=1024), dict(nm=[128, 129], pred_fresh=[0, 1], layout=[[1, 0, 0], [2, 2, 0]], comm=[0, 1])),
    ("pred_kind", ["caps", "markers"], {}, dict(nm=[1, 2, 4], pred_kind_req=[0, 1, 2, 3], threads_req=[0, 64])),
    ("eh_modes", ["markers"], {}, dict(pred_kind_req=[0, 3], eh_modes=[0, 1, 2])),
    # fused solve
    ("fuse_chain", ["caps"], dict(nparticle_max=200001), dict(fuse_solve=[0, 1, 2], nx=[1024, 1025, 3074, 3075], chain_mfma=[0, 1])),
    ("fuse_npe", ["caps"], {}, dict(fuse_solve=[1, 2], field_npe=[1, 32, 33], nx=[32, 1025])),
    ("moment", ["whole"], {}, dict(pending=[0, 1], steps_left=[1, 2, 3], output_now=[0, 1], output_next=[0, 1], optimize_now=[0, 1],
                                   optimize_next=[0, 1], fuse_output=[0, 2])),
    ("moment_no_fuse", ["whole"], dict(fuse_solve=0), dict(pending=[0, 1], steps_left=[1, 2], have_eh=[0, 1], predict=[0, 1])),
    # outputs and diagnostics
    ("fuse_output", ["caps", "whole"], dict(steps_left=1, output_now=1, diag=1),
     dict(fuse_output=[0, 1, 2], predict=[0, 1], diag_sum=[0, 1], charge_sum=[0, 1])),
    # carry and field solve
    ("carry", ["carry"], {}, dict(carry=[-1, 0, 1, 2], iptcldist=[0, 1, 2, 3], pow2=[[0, 0], [1, 0]], one_exp=[[0, 0], [1, 0]],
                                  physics=PHYSICS, launch=LAUNCHES)),
    ("field_paths", ["caps", "solve", "whole"], {}, dict(field_solver=[0, 1], field_transform=[0, 1], pred_fresh=[0, 1], pending=[0, 1])),
    # streaming
    ("streaming", ["markers"], dict(nx=1024), dict(nparticle_max=[NT_FULL, NT_FULL + 1, NT_HALF, NT_HALF + 1], full=[0, 1], pred=[0, 1])),
    ("nt_force", ["markers"], dict(nx=1024), dict(nt_force=[-1, 0, 1, 2, 3], full=[0, 1], nparticle_max=[1001, NT_FULL + 1])),
    # ranks and the tail
    ("tail", ["markers"], {}, dict(tail_on=[0, 1], ranks=RANKS, tail_ok=[0, 1], pred_kind_req=[0, 1])),
    ("solve", ["solve"], {}, dict(pred_fresh=[0, 1], ranks=RANKS, into_E=[0, 1], tail_done=[0, 1, 2], charge_sum=[0, 1])),
    # species
    ("species", ["caps", "markers"], dict(ns=2), dict(np=[[0, 1001], [1001, 0], [0, 0], [1001, 501]], pred=[0, 1], ranks=RANKS[:3:2],
                                                      one_exp=[[0, 1], [1, 0]])),
    # the knobs, and the launch requests by hand
    ("knobs", ["caps", "whole"], {}, dict(step_mode=[0, 1], lazy_calls=[0, 1], call_pair=[0, 1], predict=[0, 1], has_pred=[-1, 0])),
    ("launch", ["markers"], {}, dict(threads_req=[0, 64], bpc_req=[0, 4], launch=LAUNCHES, nparticle_max=[4001, 10000001])),
]


def rows_of(fixed, axes):
    """the queries of a group, in the order the table stores their answers"""
    for combo in itertools.product(*axes.values()):
        q = dict(fixed)
        for name, v in zip(axes, combo):
            q.update(v if isinstance(v, dict) else {name: v})
        yield q


def flat(a, sections, ns):
    """what a row stores of an answer: the integers of its sections in the order of include/pic1dp_probe.h, the names last"""
    sp = a["markers"]["species"][:ns]
    v = []
    for sec in sections:
        if sec == "markers":
            v += [a["markers"][n] for n in a["markers"] if n != "species"]
            for L in sp:
                v += [L[n] for n in L if n != "name"]
        elif sec == "carry":
            v += [L["carry"] for L in sp]
        else:
            v += list(a[sec].values())
    return v + ([L["name"] for L in sp] if "markers" in sections else [])


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_plan.json")
    dump = lambda v: json.dumps(v, separators=(",", ":"))
    head = dict(base=BASE, turning=dict(nx_step=NX_STEP, nx_step_exact=NX_STEP_EXACT, nxo_diag=NXO_DIAG, nt_full=NT_FULL, nt_half=NT_HALF))
    nrows = 0
    with open(out, "w") as f:
        f.write("{" + ",\n".join(json.dumps(k) + ":" + dump(v) for k, v in head.items()) + ',\n"groups":[\n')
        for i, (name, sections, fixed, axes) in enumerate(GROUPS):
            want = [flat(answer(q), sections, dict(BASE, **q)["ns"]) for q in rows_of(fixed, axes)]
            nrows += len(want)
            lines = [",".join(dump(w) for w in want[j:j + 16]) for j in range(0, len(want), 16)]     # sixteen answers per line
            f.write(dump(dict(name=name, sections=sections, fixed=fixed, axes=axes))[:-1] + ',"want":[\n' + ",\n".join(lines) + "\n]}" +
                    (",\n" if i + 1 < len(GROUPS) else "\n"))
        f.write("]}\n")
    json.load(open(out))
    print(out, nrows, "rows", os.path.getsize(out), "bytes")
