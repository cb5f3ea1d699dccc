"""ms per pic1dp_hip_zoom call (include/pic1dp_hip.h) on the window v in [3, 5] over the whole box, which = 7,
in the three forms the plan knows -- one pass with the planes in LDS (64 x 64), band passes (512 columns, 2, 4, 8 and 16
passes of 12 rows) and one pass straight into memory on the same grids -- and beside them, from the same process, figures of
code the call does not touch: the probe library's pure read stream of the same arrays (include/pic1dp_probe.h
pic1dp_probe_stream) and the wall clock of pic1dp_hip_select of the same window plus numpy.histogram2d on the host.

Every (library, round) is a fresh child process under its own `timeout -k 10`.  A child loads the markers on the device,
takes one step between two records (the caches hold what a run would leave there), waits, and times the call alone: the
median of the wall clock around the synchronous call, and the mean device time of a call's passes over the same records from
zoom_stats().  The banded and the memory form of one grid alternate inside the child: banded, memory, banded, memory.  A
child that fails, faults or times out ends the tool: nothing more is started on the GPU.

    python tools/zoom_bench.py [--rounds 3] [--case C3] [--libs A.so,B.so]

Which form a grid takes is the plan's decision (csrc/launch_policy.hpp kZoomPassCap).  Only a tuning build
(PIC1DP_EXTRA_FLAGS=-DPIC1DP_TUNING) reads PIC1DP_ZOOM_PASS_CAP, which this tool sets per call to force
either form; with the default build every grid is measured in the form the plan gives it, twice.  --libs: libraries to
load (PIC1DP_LIB), alternating round by round -- a build with -DPIC1DP_ZOOM_SKIP=1 against one without, say.
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
V = (3.0, 5.0)
BANDS = (2, 4, 8, 16)


def child(case, records=5, warm=1):
    sys.path.insert(0, ROOT)
    import numpy as np

    import pic1dp_amd as amd
    from pic1dp_amd import probe
    kw = CASES[case]
    n = kw["nparticle_max"]
    eng = amd.Pic1dp(amd.make_input(**kw), device=0)
    eng.particle_load_device(1)
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    eng.kernel_stats_enable(True)
    lx = eng.inp.lx
    out = dict(case=case, markers=n, nx=kw["nx"], tuning_build=bool(amd.tuning_build()), lib=os.environ.get("PIC1DP_LIB", ""))
    out["in_window"] = eng.select_count(0, v=V)

    def timed(call, cap=None):
        """(median wall ms, mean device ms of the zoom passes, passes) per call over the timed records"""
        if cap is not None:
            os.environ["PIC1DP_ZOOM_PASS_CAP"] = str(cap)
        ms = []
        for r in range(warm + records):
            if r == warm:
                d0, n0, _ = eng.zoom_stats()
            eng.step(1)
            eng.sync()
            t0 = time.perf_counter()
            call()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warm:
                ms.append(dt)
        d1, n1, _ = eng.zoom_stats()
        os.environ.pop("PIC1DP_ZOOM_PASS_CAP", None)
        return statistics.median(ms), (d1 - d0) / records, (n1 - n0) / records

    def zoom(bins, which=7):
        return lambda: eng.zoom(0, x=(0.0, lx), v=V, bins=bins, which=which)

    wall, dev, passes = timed(zoom((64, 64)))
    out.update(lds_ms=wall, lds_device_ms=dev, lds_passes=passes)
    wall, dev, passes = timed(zoom((64, 64), 1))
    out.update(lds_markr_ms=wall, lds_markr_device_ms=dev)
    for k in BANDS:
        bins = (512, 12 * k)            # three planes of 512 columns: 19 200 / 1536 = 12 rows a pass
        b1, m1 = timed(zoom(bins), 64), timed(zoom(bins), 1)
        b2, m2 = timed(zoom(bins), 64), timed(zoom(bins), 1)
        out["banded%d_device_ms" % k] = 0.5 * (b1[1] + b2[1])
        out["banded%d_ms" % k] = 0.5 * (b1[0] + b2[0])
        out["banded%d_passes" % k] = b1[2]
        out["memory%d_device_ms" % k] = 0.5 * (m1[1] + m2[1])
        out["memory%d_ms" % k] = 0.5 * (m1[0] + m2[0])
        out["memory%d_passes" % k] = m1[2]
    wall, dev, passes = timed(zoom((512, 512)))
    out.update(zoom512_ms=wall, zoom512_device_ms=dev, zoom512_passes=passes)

    def select_and_histogram():
        g = eng.select(0, v=V)
        px = np.fmod(g["x"], lx)
        px = np.where(px < 0.0, px + lx, px)
        for wts in (None, g["p"], g["w"]):
            np.histogram2d(g["v"], px, bins=(512, 512), range=(V, (0.0, lx)), weights=wts)

    ms = []
    for r in range(3):
        eng.step(1)
        eng.sync()
        t0 = time.perf_counter()
        select_and_histogram()
        ms.append((time.perf_counter() - t0) * 1e3)
    out["select_histogram2d_ms"] = statistics.median(ms)
    eng.close()
    out["read_stream4_gb_per_s"] = probe.stream(4, 0, n, reps=10)
    out["read_stream2_gb_per_s"] = probe.stream(2, 0, n, reps=10)
    out["read_stream1_gb_per_s"] = probe.stream(1, 0, n, reps=10)
    out["lds_fraction_of_read_stream"] = 32.0 * n / (out["lds_device_ms"] * 1e6) / out["read_stream4_gb_per_s"]
    out["lds_markr_fraction_of_read_stream"] = 16.0 * n / (out["lds_markr_device_ms"] * 1e6) / out["read_stream2_gb_per_s"]
    for k in BANDS:
        out["banded%d_pass_fraction_of_read_stream" % k] = 32.0 * n * k / (out["banded%d_device_ms" % k] * 1e6) / out["read_stream4_gb_per_s"]
    print(json.dumps(out))


def run(args, limit, lib):
    env = dict(os.environ)
    if lib:
        env["PIC1DP_LIB"] = os.path.abspath(lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        print(json.dumps(dict(stopped=args, lib=lib, returncode=r.returncode)))
        sys.exit(1)    # a failed, faulted or timed-out child: nothing more on the GPU
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--case", default="C3")
    ap.add_argument("--libs", default="", help="libraries to load (PIC1DP_LIB), alternating round by round")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    libs = a.libs.split(",") if a.libs else [""]
    rows = {lib: [] for lib in libs}
    for rnd in range(a.rounds):
        for lib in libs:
            r = run(["--child", a.case], 280, lib)
            print(json.dumps(dict(round=rnd, **r)), flush=True)
            rows[lib].append(r)
    for lib in libs:
        keys = [k for k in rows[lib][0] if isinstance(rows[lib][0][k], float)]
        print(json.dumps(dict(summary=a.case, lib=lib, median={k: statistics.median(r[k] for r in rows[lib]) for k in keys},
                              round_to_round_spread={k: max(r[k] for r in rows[lib]) - min(r[k] for r in rows[lib]) for k in keys})), flush=True)


if __name__ == "__main__":
    main()
