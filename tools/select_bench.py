"""ms per pic1dp_hip_select_count, pic1dp_hip_select and pic1dp_hip_gather call (include/pic1dp_hip.h) at C3
(1e8 markers, nx 1024, after ten steps), and beside them, from the same process, the two figures they are held against:
the probe library's pure read stream of TWO arrays of the same length through the same tiles (16 B per marker,
include/pic1dp_probe.h pic1dp_probe_stream) -- the yardstick of the count pass, taken twice that of a selection -- and the
same 2^20 markers obtained the old way: pic1dp_hip_particles_download of four arrays and a numpy mask.

Every round is a fresh child process under its own `timeout -k 10`.  A child loads the markers on the device, takes ten
steps, and times each call alone: the median and the spread (max - min) of the wall clock around the synchronous call over
nine repeats after two warm-up calls, and the mean device time of a call's passes over the same repeats from
kernel_stats(21) / kernel_stats(22).  The selection is a window in v around the resonance thinned to about 2^20 markers;
the gather takes 2^20 random indices.  A child that fails, faults or times out ends the tool: nothing more is started on
the GPU.

    python tools/select_bench.py [--rounds 3] [--markers 100000000] [--nx 1024]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = 1 << 20


def child(markers, nx, repeats=9, warm=2):
    sys.path.insert(0, ROOT)
    import numpy as np

    import pic1dp_amd as amd
    from pic1dp_amd import probe
    n = markers
    eng = amd.Pic1dp(amd.make_input(nparticle_max=n, nx=nx), device=0)
    eng.particle_load_device(1)
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    eng.step(10)
    eng.sync()
    eng.kernel_stats_enable(True)
    lx = eng.inp.lx
    out = dict(markers=n, nx=nx)

    def timed(call, stat):
        """(median wall ms, spread of the wall ms, mean device ms, passes per call) over the timed repeats"""
        ms = []
        for r in range(warm + repeats):
            if r == warm:
                d0, n0 = eng.kernel_stats(stat)
            t0 = time.perf_counter()
            call()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warm:
                ms.append(dt)
        d1, n1 = eng.kernel_stats(stat)
        return statistics.median(ms), max(ms) - min(ms), (d1 - d0) / repeats, (n1 - n0) / repeats

    # a window in v around the bump's resonance, thinned so that about 2^20 markers remain
    window = dict(v=(3.0, 4.0))
    in_window = eng.select_count(0, **window)
    fraction = min(1.0, TARGET / max(in_window, 1))
    sel = dict(window, fraction=fraction, key=1)
    out["in_window"] = in_window
    out["selected"] = eng.select_count(0, **sel)

    for name, call, stat in (("select_count", lambda: eng.select_count(0, **sel), 21),
                             ("select", lambda: eng.select(0, max=2 * TARGET, **sel), 21),
                             ("select_thinned_everywhere", lambda: eng.select(0, max=2 * TARGET, fraction=TARGET / n, key=1), 21)):
        wall, spread, dev, passes = timed(call, stat)
        out[name + "_ms"], out[name + "_ms_spread"], out[name + "_device_ms"], out[name + "_passes"] = wall, spread, dev, passes
    idx = np.random.default_rng(1).integers(0, n, TARGET)
    wall, spread, dev, passes = timed(lambda: eng.gather(0, idx), 22)
    out["gather_ms"], out["gather_ms_spread"], out["gather_device_ms"], out["gather_entries"] = wall, spread, dev, TARGET

    # the old way to the same markers: every marker over PCIe, then a mask on the host
    def old_way():
        g = eng.particles_download(0)
        m = np.nonzero((g["v"] >= 3.0) & (g["v"] < 4.0))[0]
        return {k: a[m] for k, a in g.items()}
    ms = []
    for r in range(3):
        t0 = time.perf_counter()
        old_way()
        ms.append((time.perf_counter() - t0) * 1e3)
    out["download_and_mask_ms"], out["download_and_mask_ms_spread"] = statistics.median(ms), max(ms) - min(ms)
    eng.close()

    gbs = probe.stream(2, 0, n, reps=10)
    out["read_stream_2_arrays_gb_per_s"] = gbs
    stream_ms = 16.0 * n / (gbs * 1e6)
    out["read_stream_ms"] = stream_ms
    out["select_count_fraction_of_read_stream"] = stream_ms / out["select_count_device_ms"]
    out["select_fraction_of_two_read_streams"] = 2.0 * stream_ms / out["select_thinned_everywhere_device_ms"]
    out["select_speedup_over_download_and_mask"] = out["download_and_mask_ms"] / out["select_ms"]
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
    ap.add_argument("--markers", type=int, default=100_000_000)
    ap.add_argument("--nx", type=int, default=1024)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.markers, a.nx)
    rows = []
    for rnd in range(a.rounds):
        r = run(["--child", "--markers", str(a.markers), "--nx", str(a.nx)], 280)
        print(json.dumps(dict(round=rnd, **r)), flush=True)
        rows.append(r)
    keys = [k for k in rows[0] if isinstance(rows[0][k], float)]
    print(json.dumps(dict(summary="select", median={k: statistics.median(r[k] for r in rows) for k in keys},
                          round_to_round_spread={k: max(r[k] for r in rows) - min(r[k] for r in rows) for k in keys})), flush=True)


if __name__ == "__main__":
    main()
