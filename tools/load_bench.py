#!/usr/bin/env python3
"""load_bench.py -- what the initial condition costs: wall clock of pic1dp_hip_particle_load (host generator, 32 B per
marker over PCIe) against pic1dp_hip_particle_load_device(1) and (2), and the device time of k_load against the probe
library's four-array write stream of the same size in the same session.  Every figure comes from a fresh
child process; the rounds alternate host | random | quiet | stream.
    python tools/load_bench.py [markers] [nx] [rounds]        (default: C3 = 1e8 markers, nx 1024, 3 rounds)
    python tools/load_bench.py --child host|random|quiet|stream markers nx"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KINDS = {"host": 0, "random": 1, "quiet": 2}


def child(what, n, nx):
    if what == "stream":
        from pic1dp_amd import probe
        probe.write_stream(n, reps=3)                                  # (first launches: code loading)
        print(json.dumps({"what": what, "gbs": probe.write_stream(n, reps=10)}))
        return
    import pic1dp_amd
    eng = pic1dp_amd.Pic1dp(pic1dp_amd.make_input(nparticle_max=n, nx=nx))
    eng.kernel_stats_enable(True)
    wall, dev = [], []
    for _ in range(3):                                                 # the first call pays code loading and first touch
        ms0 = eng.kernel_stats(19)[0]
        eng.sync()
        t0 = time.perf_counter()
        if KINDS[what]:
            eng.particle_load_device(KINDS[what])
        else:
            eng.particle_load()
        eng.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(eng.kernel_stats(19)[0] - ms0)
    print(json.dumps({"what": what, "wall_ms": wall, "k_load_ms": dev}))


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10**8
    nx = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    res = {k: [] for k in ("host", "random", "quiet", "stream")}
    for _ in range(rounds):
        for what in res:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(n), str(nx)], check=True,
                                 capture_output=True, text=True, timeout=600).stdout
            res[what].append(json.loads(out.strip().splitlines()[-1]))
    med = lambda v: sorted(v)[len(v) // 2]
    stream = med([r["gbs"] for r in res["stream"]])
    print("%d markers, nx %d, %d rounds of fresh processes (median of the rounds; per process: first call | best later call)" % (n, nx, rounds))
    print("write stream of four arrays (probe library)   %.0f GB/s" % stream)
    for what in ("host", "random", "quiet"):
        first = med([r["wall_ms"][0] for r in res[what]])
        later = med([min(r["wall_ms"][1:]) for r in res[what]])
        line = "%-7s wall clock first call %9.2f ms | later %9.2f ms" % (what, first, later)
        if what != "host":
            k = med([min(r["k_load_ms"][1:]) for r in res[what]])
            gbs = 32.0 * n / (k * 1e-3) / 1e9 if k > 0 else 0.0
            line += " | k_load %.3f ms = %.0f GB/s written = %.2f of the stream" % (k, gbs, gbs / stream if stream else 0.0)
        print(line)
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        main()
