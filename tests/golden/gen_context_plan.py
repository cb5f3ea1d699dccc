"""tests/golden/context_plan.json: what pic1dp_hip_create decides before its first allocation, transcribed from create()'s
own formulas as they stood in capi.cpp (with block_alloc / block_np of loader.cpp and the LDS sizes of kernels.hpp) before
context_plan.cpp took them over.  Run once; tests/test_context_plan_host.py reads the table.
    python tests/golden/gen_context_plan.py"""
import itertools
import json
import os

PARTICLE_LDS_CAP = 159 * 1024
CU_LDS, STATIC_LDS = 160 * 1024, 1024
PRED_MAX_MODES, PRED_SUM_COPIES, PRIV_THREADS = 3, 16, 768
NPARTICLE_MAX = 200005            # divides by neither 2 nor 8, and the second of two ranks owns blocks of both sizes
NPARTICLE_INIT = [200005, 150001]  # the second species leaves slots unloaded, their number no multiple of 8 either


def even(n):
    return (n + 2) & ~1


def step_sums_lds_bytes(nx):
    return 8 * (3 * even(nx) + even(nx) + 96)


def step_one_lds_bytes(nx, nm):
    return 8 * (2 * even(nx) + (nx + 1) * 2 * nm + even(nx) + (nx + 2) * (1 + 2 * nm) + 2)


def step_one_private_lds_bytes(nx):
    return 8 * (2 * even(nx) + (nx + 1) * 2 + even(nx) + 6 * PRIV_THREADS + 16)


def last_fit(fits):
    """the largest nx for which fits(nx) holds (fits is monotone)"""
    nx = 1
    while fits(nx + 1):
        nx += 1
    return nx


def turning_points():
    pts = [1, 7, 8, 192, 256, 257, 1024, 1096, 1097]
    for nm in (1, 2, 3):
        n = last_fit(lambda nx: step_one_lds_bytes(nx, nm) <= PARTICLE_LDS_CAP)
        pts += [n, n + 1]
    n = last_fit(lambda nx: step_sums_lds_bytes(nx) <= PARTICLE_LDS_CAP)
    pts += [n, n + 1]
    return sorted(set(pts))


def block_alloc(nglobal, rank, size):
    return nglobal // size + (1 if nglobal % size > rank else 0)


def block_np(nmax, ninit, mype, npe):
    spare = nmax - ninit
    unload = spare // npe + (spare % npe if mype == 0 else 0)
    return block_alloc(nmax, mype, npe) - unload


def plan(nx, nm, ns, pred_req=0, gcopies_req=0, layout=(1, 0, 0), one_rank_order=0, opt=(0, 0, 0)):
    nranks, npe, rank = layout
    if npe <= 0:
        npe = nranks
    nblk = npe // nranks
    blk0 = rank * nblk
    blk_alloc = [block_alloc(NPARTICLE_MAX, blk0 + b, npe) for b in range(nblk)]
    blk_np = [[block_np(NPARTICLE_MAX, NPARTICLE_INIT[s], blk0 + b, npe) for b in range(nblk)] for s in range(ns)]
    gcopies = 8 if nx <= 256 else 1
    k = gcopies_req
    if 1 <= k <= 64 and (k & (k - 1)) == 0:
        gcopies = k
    private_fits = 2 * (step_one_private_lds_bytes(nx) + STATIC_LDS) <= CU_LDS
    tiles_fit = nm <= PRED_MAX_MODES and step_one_lds_bytes(nx, nm) <= PARTICLE_LDS_CAP
    sums_fit = nm == 1 and nx >= 8 and step_sums_lds_bytes(nx) <= PARTICLE_LDS_CAP
    kind = 0
    if tiles_fit:
        kind = 1
    elif sums_fit:
        kind = 2
    if kind == 1 and nm == 1 and nx >= 8 and private_fits:
        kind = 2
    in_registers = False
    if pred_req in (2, 3) and sums_fit:
        kind = 2
    if pred_req == 3:
        in_registers = True
    if pred_req == 1 and tiles_fit:
        kind = 1
    private = int(kind == 2 and private_fits and not in_registers)
    pred_set = 0 if kind == 0 else (8 * PRED_SUM_COPIES if kind == 2 else ns * (1 + 2 * nm) * nx)
    pack = 0 if kind == 0 else (nx + 8 if kind == 2 else (2 + 2 * nm) * nx)
    return {"npe": npe, "nblk": nblk, "blk0": blk0, "nalloc": sum(blk_alloc), "imerge": int(opt[0] > 0), "iremove": int(opt[1] > 0),
            "isplit": int(opt[2] > 0), "gcopies": gcopies, "gstride": ns * nx, "rho_set_doubles": gcopies * ns * nx,
            "pred_kind": kind, "pred_private": private, "pred_set_doubles": pred_set, "pack_doubles": pack,
            "tab_lds": int(2 * nm * nx * 8 <= 96 * 1024), "field_npe": 1 if one_rank_order else npe,
            "np": [sum(r) for r in blk_np], "blk_alloc": blk_alloc, "blk_np": blk_np, "sc_re": 1.0 / nx, "sc_im": -1.0 / nx}


LAYOUTS = [(1, 0, 0), (1, 8, 0), (2, 8, 1), (8, 8, 7)]
PRED_REQ = [0, 1, 2, 3]
GCOPIES_REQ = [0, 4, 3, 128]   # none, honoured, refused (no power of two), refused (beyond 64)
OPT = [(0, 0, 0), (2, 0, 1), (0, 3, 0)]
QUERY = ("nx", "nm", "ns", "pred_req", "gcopies_req", "layout", "one_rank_order", "opt")
PLAN = ("npe", "nblk", "blk0", "nalloc", "imerge", "iremove", "isplit", "gcopies", "gstride", "rho_set_doubles", "pred_kind",
        "pred_private", "pred_set_doubles", "pack_doubles", "tab_lds", "field_npe", "np", "blk_alloc", "blk_np")


def table():
    nxs = turning_points()
    rows = []

    def add(nx, nm, ns, pred_req=0, gcopies_req=0, layout=(1, 0, 0), one_rank_order=0, opt=(0, 0, 0)):
        q = (nx, nm, ns, pred_req, gcopies_req, list(layout), one_rank_order, list(opt))
        p = plan(nx, nm, ns, pred_req, gcopies_req, layout, one_rank_order, opt)
        assert p["sc_re"] == 1.0 / nx and p["sc_im"] == -1.0 / nx     # (recorded once per grid below)
        rows.append([list(q), [p[k] for k in PLAN]])

    # which one-pass kernel: every grid x kept modes x request; a second species where nothing is asked for
    for nx, nm, req in itertools.product(nxs, (1, 2, 3, 4), PRED_REQ):
        add(nx, nm, 1, pred_req=req)
    for nx, nm in itertools.product(nxs, (1, 2, 3, 4)):
        add(nx, nm, 2)
    # the accumulators' copies: both sides of nx 256 x override
    for nx, ns, g in itertools.product((192, 256, 257, 1024), (1, 2), GCOPIES_REQ):
        add(nx, 1, ns, gcopies_req=g)
    # blocks and slots, the field's summation order: every layout x species; the optimisation counters
    for lay, ns, one in itertools.product(LAYOUTS, (1, 2), (0, 1)):
        add(192, 1, ns, layout=lay, one_rank_order=one)
    for opt in OPT[1:]:
        add(192, 1, 1, opt=opt)
    return {"nparticle_max": NPARTICLE_MAX, "nparticle_init": NPARTICLE_INIT, "nx": nxs, "query": QUERY, "plan": PLAN,
            "sc": [[1.0 / nx, -1.0 / nx] for nx in nxs], "rows": rows}


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "context_plan.json")
    t = table()
    dump = lambda v: json.dumps(v, separators=(",", ":"))
    lines = [",".join(dump(r) for r in t["rows"][i:i + 8]) for i in range(0, len(t["rows"]), 8)]
    with open(out, "w") as f:     # eight rows [query, plan] per line
        f.write("{" + ",\n".join(json.dumps(k) + ":" + dump(v) for k, v in t.items() if k != "rows"))
        f.write(',\n"rows":[\n' + ",\n".join(lines) + "\n]}\n")
    print(out, len(t["rows"]), "rows")
