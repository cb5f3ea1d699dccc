"""tests/golden/diag_launch.json: the launch shapes of output_all's diagnostics passes and the scales of their fixed-point
sums, transcribed from the launchers' own formulas as they stood in kernels_diag.hip and capi_diag.cpp before
launch_policy.cpp took them over (ptcldist_blocks, launch_ptcldist, ptcldist_exact_blocks, ptcldist_exact_lds,
launch_ptcldist_exact, the tail-slot block count, make_dist_scale).  Run once; tests/test_diag_launch_host.py reads the table.
    python tests/golden/gen_diag_launch.py"""
import json
import math
import os

GRIDS = [[64, 64], [80, 79], [80, 80], [79, 80], [40, 200], [16, 16], [1, 2]]
NP = [1, 2, 2047, 2048, 2049, 2**17 - 1, 2**17, 2**18 + 1, 9437184, 9437185, 10**8]
NUM_CU = [8, 256]
NTAIL = [0, 1, 256, 257, 262143, 262144, 262145, 10**8]
BOUNDS = [[0.0, 1.0], [1.0, 0.0], [1.0, 1.0], [3.5e-7, 0.02], [1.0, float("inf")], [float("inf"), 1.0], [2.0**-980, 1.0],
          [1.0, 2.0**990], [0.5, 4.0], [-1.0, 1.0]]
SCALE_NP = [1, 4097, 6400000, 10**8]
SCALE_BLOCKS = [0, 1, 256]
THREADS = [256, 1024]


def fp64_pass(np_, nxo, nvo, num_cu):
    hist = 8 * (3 * nxo * nvo + 3 * nvo)
    lds = hist <= 150 * 1024
    blocks = max(1, min(num_cu if lds else 2 * num_cu, ((np_ >> 1) + 1023) // 1024))
    return [blocks, 1024, int(lds), (hist if lds else 0) + 18 * 8, int(32.0 * np_ > 288.0 * 1048576.0)]


def exact_pass(np_, nxo, nvo, num_cu):
    lds = 8 * (3 * nxo * nvo + 8) <= 150 * 1024
    blocks = max(1, min(np_ >> 17, num_cu))
    return [blocks, 1024, int(lds), 8 * ((3 * nxo * nvo if lds else 0) + 8), int(32.0 * np_ > 288.0 * 1048576.0)]


def tail_blocks(ntail):
    return min(1024, (ntail + 255) // 256) if ntail > 0 else 0


def dist_scale(np_, blocks, deltaf, bp, bw, threads):
    use = blocks > 0 and bp > 0.0 and (not deltaf or bw > 0.0) and math.isfinite(bp) and math.isfinite(bw)
    e = [0, 0, 0]
    if use:
        per_wg = 2.0 * threads * math.ceil(float((np_ >> 1) + 1) / (float(blocks) * threads)) + 2.0
        e_n = int(math.ceil(math.log2(per_wg))) + 1
        for k, b in enumerate([1.0, bp, bw if deltaf else 1.0]):
            eb = math.frexp(b)[1]
            e[k] = min(62 - e_n, 50) - eb
            if e[k] < -900 or e[k] > 900:
                use = False
    return [int(use)] + e


def table():
    rows = {"fp64": [], "exact": []}
    for nxo, nvo in GRIDS:
        for np_ in NP:
            for cu in NUM_CU:
                rows["fp64"].append(fp64_pass(np_, nxo, nvo, cu))
                rows["exact"].append(exact_pass(np_, nxo, nvo, cu))
    scale = [dist_scale(np_, b, d, bp, bw, th) for np_ in SCALE_NP for b in SCALE_BLOCKS for d in (0, 1) for bp, bw in BOUNDS
             for th in THREADS]
    js = lambda x: "inf" if x == float("inf") else x
    return {"grids": GRIDS, "np": NP, "num_cu": NUM_CU, "rows": rows, "ntail": NTAIL, "tail_blocks": [tail_blocks(n) for n in NTAIL],
            "bounds": [[js(a), js(b)] for a, b in BOUNDS], "scale_np": SCALE_NP, "scale_blocks": SCALE_BLOCKS,
            "threads": THREADS, "scale": scale}


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "diag_launch.json")
    with open(out, "w") as f:
        json.dump(table(), f, separators=(",", ":"))
        f.write("\n")
    print(out)
