#!/usr/bin/env python
"""A/B of library builds on ONE box, as profiles/r23/ab_sweep.log was taken: `python bench.py --steps 100 --warmup 40
--repeats 5 [workload]` in alternating fresh processes, N runs each, a line per run and SUMMARY lines (median, min, max,
spread = max - min of the runs' ms per step) per workload and build.

    python tools/ab_trims.py --runs 4 --workloads headline,c2,share  parent=/path/parent.so  new=
    python tools/ab_trims.py --runs 4 --workloads headline  P=/p/tune_P.so  A=/p/tune_A.so  B=/p/tune_P.so:PIC1DP_PLAIN_ROWS=1 \\
                                                            AB=/p/tune_A.so:PIC1DP_PLAIN_ROWS=1

A build is label=library[:NAME=VALUE ...]; an empty library is the tree's own.  The 2 x 2 of DESIGN.md 8 (round 29) is the
second call, with -DPIC1DP_TUNING builds of the tree with and without -DPIC1DP_TRIMS=0.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {"headline": [], "c2": ["--config", "c2"], "share": ["--particles", "12500000"],
             # through the three call sites per sub-step (round 31: what a call's plan costs the host)
             "c2_calls": ["--config", "c2", "--unfused"], "small_calls": ["--unfused", "--particles", "200000"]}


def find(d, key):
    if isinstance(d, dict):
        if key in d and not isinstance(d[key], (dict, list)):
            return d[key]
        for v in d.values():
            r = find(v, key)
            if r is not None:
                return r
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--workloads", default="headline,c2,share")
    ap.add_argument("--timeout", type=int, default=240, help="seconds one bench.py process may take")
    ap.add_argument("builds", nargs="+")
    a = ap.parse_args()
    builds = []
    for b in a.builds:
        label, _, rest = b.partition("=")
        parts = rest.split(":")
        builds.append((label, parts[0], dict(p.split("=", 1) for p in parts[1:])))
    print("# python bench.py --steps 100 --warmup 40 --repeats 5 [workload], alternating fresh processes, %d runs each: %s"
          % (a.runs, "  ".join("%s = %s %s" % (l, os.path.basename(p) or "this tree's library", " ".join("%s=%s" % kv for kv in e.items()))
                              for l, p, e in builds)), flush=True)
    ms = {}
    for w in a.workloads.split(","):
        for run in range(a.runs):
            for label, lib, extra in builds:
                env = dict(os.environ, **extra)
                env.pop("PIC1DP_LIB", None)
                if lib:
                    env["PIC1DP_LIB"] = lib
                r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "40",
                                    "--repeats", "5"] + WORKLOADS[w], env=env, capture_output=True, text=True, timeout=a.timeout)
                if r.returncode != 0:   # nothing more is started on this GPU
                    print("%s %s run %d FAILED (exit %d)\n%s" % (w, label, run, r.returncode, r.stderr[-2000:]), flush=True)
                    return 1
                res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                t = res["ms_per_step"]
                ms.setdefault((w, label), []).append(t)
                print("%-8s %-6s run %d  ms_per_step %.5f  (blocks min %.5f max %.5f)  kernel %.5f ms  field_energy_end %r"
                      % (w, label, run, t, res["ms_per_step_min"], res["ms_per_step_max"], find(res, "avg_launch_ms") or float("nan"),
                         find(res, "field_energy_end")), flush=True)
    for (w, label), v in sorted(ms.items()):
        print("SUMMARY %-8s %-6s median %.5f  min %.5f  max %.5f  spread %.5f" % (w, label, statistics.median(v), min(v), max(v), max(v) - min(v)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
