"""ms per pic1dp_hip_power call (include/pic1dp_hip.h), which = 2 (the w plane) and 3 (both sets), and
beside them, from the same process, two figures of code the call does not touch: kind 0's output_all -- whose marker pass is
k_ptcldist, the kernel k_power is shaped after -- and the probe library's pure read stream of four arrays of the same length
(include/pic1dp_probe.h pic1dp_probe_stream).

Every (case, round) is a fresh child process under its own `timeout -k 10`.  A child loads the markers, takes one step
between two records (the caches hold what a run would leave there), waits, and times the call alone, nine records after
two warm-up records: the median of the wall clock around the synchronous call, and the mean device time of a call's passes
over the same nine records from kernel_stats(20).  output_all has no device clock of its own: its figure is the wall clock
around the call (the pass, int E^2 dx, the record's packing and one transfer); a kernel trace of one child gives k_ptcldist's
device time where it is wanted.  A child that fails, faults or times out ends the tool: nothing more is started on the GPU.

    python tools/power_bench.py [--rounds 5] [--cases C3,C1] [--exact]

--exact measures pic1dp_hip_power_exact (device time from power_exact_stats()) alternately with kind 0 in the
same child -- kind 0, exact, kind 0, exact for which = 2, then for which = 3 -- and adds the ratio exact / kind 0 of the
device times (the mean of the two kind-0 measurements below it) and the exact passes' share of the read stream.
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


def child(case, exact=False, records=9, warm=2):
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
    out = dict(case=case, markers=n, nx=kw["nx"], nx_opd=eng.inp.nx_opd, nv_opd=eng.inp.nv_opd)

    def stats(stat):   # kind 0: kernel_stats(20); the exact kind has an entry point of its own
        return eng.kernel_stats(stat) if stat != "exact" else eng.power_exact_stats()[:2]

    def timed(call, stat=20):
        """(median wall ms, mean device ms of the power passes, passes) per call over the timed records"""
        ms = []
        for r in range(warm + records):
            if r == warm:
                d0, n0 = stats(stat)
            eng.step(1)
            eng.sync()
            t0 = time.perf_counter()
            call()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warm:
                ms.append(dt)
        d1, n1 = stats(stat)
        return statistics.median(ms), (d1 - d0) / records, (n1 - n0) / records

    for which in (2, 3):
        wall, dev, passes = timed(lambda: eng.power(0, which))
        if exact:   # kind 0, exact, kind 0, exact: the kind-0 figures are the means of their two measurements
            xw, xd, xp = timed(lambda: eng.power_exact(0, which), "exact")
            wall2, dev2, _ = timed(lambda: eng.power(0, which))
            xw2, xd2, _ = timed(lambda: eng.power_exact(0, which), "exact")
            wall, dev = 0.5 * (wall + wall2), 0.5 * (dev + dev2)
            out["exact%d_ms" % which] = 0.5 * (xw + xw2)
            out["exact%d_device_ms" % which] = 0.5 * (xd + xd2)
            out["exact%d_passes_per_call" % which] = xp
            out["exact%d_over_kind0_device" % which] = out["exact%d_device_ms" % which] / dev
            out["exact%d_over_kind0_wall" % which] = out["exact%d_ms" % which] / wall
        out["power%d_ms" % which] = wall
        out["power%d_device_ms" % which] = dev
        out["power%d_passes_per_call" % which] = passes
        out["power%d_device_ns_per_marker" % which] = dev * 1e6 / n
    out["output_all_ms"] = timed(eng.output_all)[0]
    out["output_all_ns_per_marker"] = out["output_all_ms"] * 1e6 / n
    eng.close()
    gbs = probe.stream(4, 0, n, reps=10)
    out["read_stream_gb_per_s"] = gbs
    for which in (2, 3):
        out["power%d_fraction_of_read_stream" % which] = BYTES[which] * n / (out["power%d_device_ms" % which] * 1e6) / gbs
        if exact:
            out["exact%d_fraction_of_read_stream" % which] = BYTES[which] * n / (out["exact%d_device_ms" % which] * 1e6) / gbs
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="C3,C1")
    ap.add_argument("--child")
    ap.add_argument("--exact", action="store_true", help="measure pic1dp_hip_power_exact beside kind 0, alternately")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.exact)
    for case in a.cases.split(","):
        rows = []
        for rnd in range(a.rounds):
            r = run(["--child", case] + (["--exact"] if a.exact else []), 300)
            print(json.dumps(dict(round=rnd, **r)), flush=True)
            rows.append(r)
        keys = [k for k in rows[0] if isinstance(rows[0][k], float)]
        print(json.dumps(dict(summary=case, median={k: statistics.median(r[k] for r in rows) for k in keys},
                              round_to_round_spread={k: max(r[k] for r in rows) - min(r[k] for r in rows) for k in keys})), flush=True)


if __name__ == "__main__":
    main()
