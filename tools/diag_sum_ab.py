"""A/B of the diagnostics sum's two kinds (include/pic1dp_hip.h set_diag_sum): ms per output_all of
  k0   kind 0, the pass as it was (fixed-point sums scaled per pass from the second record on)
  k1   kind 1, exact
each variant in a fresh child process under its own `timeout -k 10`, the variants alternating over the rounds; a
child takes one step between two records (the markers change, the cached diagnostics go), waits, and times output_all
alone; it reports the median of nine records after two warm-up records.  A child that fails, faults or times out ends
the tool: nothing more is started on the GPU.  The same file runs against a build without set_diag_sum (k0 only:
--variants k0), which is how kind 0 is compared with the commit before.

    python tools/diag_sum_ab.py [--rounds 5] [--cases C3,C1] [--variants k0,k1]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"C3": dict(nparticle_max=100_000_000, nx=1024), "C1": dict(nparticle_max=6_400_000, nx=192)}
VARIANTS = {"k0": 0, "k1": 1}


def child(case, kind, records=9, warm=2):
    sys.path.insert(0, ROOT)
    import pic1dp_amd as amd
    eng = amd.Pic1dp(amd.make_input(**CASES[case]), device=0)
    eng.particle_load()
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    if kind != 0 or hasattr(eng, "set_diag_sum"):
        eng.set_diag_sum(kind)
    ms = []
    for r in range(warm + records):
        eng.step(1)
        eng.sync()
        t0 = time.perf_counter()
        eng.output_all()
        dt = (time.perf_counter() - t0) * 1e3
        if r >= warm:
            ms.append(dt)
    print(json.dumps(dict(case=case, kind=kind, ms=statistics.median(ms), min=min(ms), max=max(ms),
                          passes=eng.kernel_stats(5)[1], fixed_point_passes=eng.kernel_stats(12)[1])))


def run(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        print(json.dumps(dict(stopped=args, returncode=r.returncode)))
        sys.exit(1)    # a failed, faulted or timed-out child: nothing more on the GPU
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="C3,C1")
    ap.add_argument("--variants", default="k0,k1")
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]))
    names = a.variants.split(",")
    res = {}
    for case in a.cases.split(","):
        for rnd in range(a.rounds):
            for name in (names if rnd % 2 == 0 else list(reversed(names))):
                r = run(["--child", case, str(VARIANTS[name])], 300)
                print(json.dumps(dict(round=rnd, variant=name, **r)), flush=True)
                res.setdefault(case, {}).setdefault(name, []).append(r["ms"])
    for case, d in res.items():
        summary = {k: statistics.median(v) for k, v in d.items()}
        spread = {k: max(v) - min(v) for k, v in d.items()}
        if "k0" in summary and "k1" in summary:
            summary["k1_over_k0"] = summary["k1"] / summary["k0"]
        print(json.dumps(dict(summary=case, ms_per_output_all=summary, round_to_round_spread_ms=spread)), flush=True)


if __name__ == "__main__":
    main()
