"""Cost of the mode-filter solve's two transforms (include/pic1dp_hip.h set_field_transform):
  solve  us per field_solve_electric from field_chargeden for nx x nmode (kept modes 1 .. nmode), transform 0 (the dense
         tables: k_field_solve for 2 nmode <= 256, else the wide pair k_field_modes_wide + k_field_inverse_wide) and
         transform 1 (k_field_fft): wall clock over `--reps` back-to-back solves behind one synchronisation, median of
         five blocks, after a warm-up block
  step   ms per step() at --markers markers, nx 1024, nmode 512, both transforms (median of five blocks of 10 steps)
One process, one context at a time.  Run it under a time limit of its own; under rocprofv3 --kernel-trace --stats the
kernel table gives the device time of each kernel.

    python tools/field_transform_bench.py [--reps 200] [--markers 100000000] [--no-step]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import pic1dp_amd as amd  # noqa: E402


def solve_us(nx, nmode, transform, reps):
    eng = amd.Pic1dp(amd.make_input(nparticle_max=16, nx=nx, nmode=nmode, modes=list(range(1, nmode + 1))), device=0)
    eng.set_field_transform(transform)
    eng.set_chargeden(np.random.default_rng(nx).standard_normal(nx))
    out = []
    for b in range(6):
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            eng.field_solve_electric()
        eng.sync()
        if b:
            out.append((time.perf_counter() - t0) * 1e6 / reps)
    eng.close()
    return statistics.median(out)


def step_ms(markers, transform, steps=10):
    eng = amd.Pic1dp(amd.make_input(nparticle_max=markers, nx=1024, nmode=512, modes=list(range(1, 513))), device=0)
    eng.particle_load()
    eng.set_field_transform(transform)
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    eng.step(steps)
    eng.sync()
    out = []
    for _ in range(5):
        t0 = time.perf_counter()
        eng.step(steps)
        eng.sync()
        out.append((time.perf_counter() - t0) * 1e3 / steps)
    eng.close()
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--markers", type=int, default=100_000_000)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    print("%6s %6s %12s %12s %8s" % ("nx", "nmode", "t0 us", "t1 us", "t0/t1"), flush=True)
    rows = []
    for nx in (192, 1024, 4096, 8192):
        for nmode in sorted({1, 16, 128, nx // 2}):
            t0 = solve_us(nx, nmode, 0, a.reps)
            t1 = solve_us(nx, nmode, 1, a.reps)
            rows.append(dict(nx=nx, nmode=nmode, t0_us=round(t0, 2), t1_us=round(t1, 2)))
            print("%6d %6d %12.2f %12.2f %8.2f" % (nx, nmode, t0, t1, t0 / t1), flush=True)
    res = dict(solve=rows)
    if not a.no_step:
        res["step_ms"] = {str(t): round(step_ms(a.markers, t), 4) for t in (0, 1)}
        print("step at %d markers, nx 1024, nmode 512: transform 0 %.4f ms, transform 1 %.4f ms"
              % (a.markers, res["step_ms"]["0"], res["step_ms"]["1"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
