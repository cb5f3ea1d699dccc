"""ms per pic1dp_hip_hermite call (include/pic1dp_hip.h): nherm 64 and 256, which = 2 with mode (1,) and
which = 3 with four modes, and beside them, from the same process, pic1dp_hip_moments which = 2 (k_moments) and the probe
library's pure read stream of four arrays of the same length (the probe has no three-array form: its rate stands beside the
which = 2 calls, which read three, as well) (include/pic1dp_probe.h pic1dp_probe_stream).

Every (case, round) is a fresh child process under its own `timeout -k 10`.  A child loads the markers, takes one step
between two records (the caches hold what a run would leave there), waits, and times the call alone, seven records after two
warm-up records: the median of the wall clock around the synchronous call, and the mean device time of the call's pass over
the same records (hermite_stats; kernel_stats(16) for the moments).  A child that fails, faults or times out ends the tool:
nothing more is started on the GPU.

    python tools/hermite_bench.py [--rounds 3] [--cases C3,C1]
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
BYTES = {2: 24, 3: 32}      # x, v and w; x, v, p and w
SPECTRA = [("w_1mode", 2, (1,)), ("pw_4modes", 3, (1, 2, 3, 4))]


def child(case, records=7, warm=2):
    sys.path.insert(0, ROOT)
    import pic1dp_amd as amd
    from pic1dp_amd import probe
    kw = CASES[case]
    n = kw["nparticle_max"]
    eng = amd.Pic1dp(amd.make_input(**kw), device=0)
    eng.particle_load()
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    eng.kernel_stats_enable(True)
    out = dict(case=case, markers=n, nx=kw["nx"])

    def timed(call, stat):
        """(median wall ms, mean device ms of the passes) per call over the timed records"""
        ms = []
        for r in range(warm + records):
            if r == warm:
                d0 = stat()[0]
            eng.step(1)
            eng.sync()
            t0 = time.perf_counter()
            call()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warm:
                ms.append(dt)
        return statistics.median(ms), (stat()[0] - d0) / records

    for name, which, modes in SPECTRA:
        for nherm in (64, 256):
            key = "hermite_%s_n%d" % (name, nherm)
            out[key + "_ms"], out[key + "_device_ms"] = timed(lambda: eng.hermite(0, modes, nherm, 0.0, 1.0, which), eng.hermite_stats)
    out["moments2_ms"], out["moments2_device_ms"] = timed(lambda: eng.moments(0, 2), lambda: eng.kernel_stats(16))
    eng.close()
    # the probe streams 1, 2, 4 or 7 arrays: the four-array stream's RATE stands beside which = 2 (three arrays: x, v, w) too,
    # as in tools/moments_bench.py; the bytes of a fraction are the call's own (24 or 32 B a marker)
    g4 = probe.stream(4, 0, n, reps=10)
    gbs = {2: g4, 3: g4}
    out["read_stream_gb_per_s"] = g4
    for name, which, _ in SPECTRA:
        for nherm in (64, 256):
            key = "hermite_%s_n%d" % (name, nherm)
            out[key + "_fraction_of_read_stream"] = BYTES[which] * n / (out[key + "_device_ms"] * 1e6) / gbs[which]
    out["moments2_fraction_of_read_stream"] = BYTES[2] * n / (out["moments2_device_ms"] * 1e6) / gbs[2]
    print(json.dumps(out))


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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="C3,C1")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    for case in a.cases.split(","):
        rows = []
        for rnd in range(a.rounds):
            r = run(["--child", case], 300)
            print(json.dumps(dict(round=rnd, **r)), flush=True)
            rows.append(r)
        keys = [k for k in rows[0] if isinstance(rows[0][k], float)]
        print(json.dumps(dict(summary=case, median={k: statistics.median(r[k] for r in rows) for k in keys},
                              round_to_round_spread={k: max(r[k] for r in rows) - min(r[k] for r in rows) for k in keys})), flush=True)


if __name__ == "__main__":
    main()
