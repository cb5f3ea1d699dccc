"""A/B of the charge sum's two kinds (include/pic1dp_hip.h set_charge_sum): ms per step of
  k0-2pass  kind 0, two passes per step (PIC1DP_PREDICT=0 in that child)
  k1        kind 1, exact (two passes per step: it predicts nothing)
  k0        kind 0 as by default (one pass per step where the prediction applies)
each variant in a fresh child process under its own `timeout -k 10`, the variants alternating over the rounds; a
child reports the median of five blocks of 20 steps.  A child that fails, faults or times out ends the tool: nothing
more is started on the GPU.  --error: kind 1's and kind 0's distance from the CPU oracle at C1 (chargeden after the
first deposit, int E^2 dx over 20 steps).

    python tools/charge_sum_ab.py [--rounds 5] [--cases C3,C1] [--error]
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
VARIANTS = {"k0-2pass": (0, {"PIC1DP_PREDICT": "0"}), "k1": (1, {}), "k0": (0, {})}


def child(case, kind, blocks=5, steps=20):
    sys.path.insert(0, ROOT)
    import pic1dp_amd as amd
    eng = amd.Pic1dp(amd.make_input(**CASES[case]), device=0)
    eng.particle_load()
    eng.set_charge_sum(kind)
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    eng.step(steps)             # warm-up
    eng.sync()
    ms = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        eng.step(steps)
        eng.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    print(json.dumps(dict(case=case, kind=kind, predict_kind=eng.predict_kind(), ms=statistics.median(ms), blocks=ms)))


def error_child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import oracle
    import pic1dp_amd as amd
    kw = CASES["C1"]
    steps = 20
    sim = oracle.Sim(oracle.make_input(**kw))
    assert sim.load() == 0
    sim.collect_charge()
    cd_o = sim.get_field()[1]
    sim.solve_field()
    e_o = [sim.field_energy()]
    for _ in range(steps):
        sim.step(1)
        e_o.append(sim.field_energy())
    out = {}
    for kind in (0, 1):
        eng = amd.Pic1dp(amd.make_input(**kw), device=0)
        eng.particle_load()
        eng.set_charge_sum(kind)
        eng.interaction_collect_charge()
        cd = eng.get_field()["chargeden"]
        eng.field_solve_electric()
        e0 = eng.field_energy()
        eng.step(steps)
        e_g = np.concatenate([[e0], eng.energy_history()])
        out["kind%d" % kind] = dict(max_rel_chargeden=float(np.max(np.abs(cd - cd_o)) / np.max(np.abs(cd_o))),
                                    max_rel_field_energy=float(np.max(np.abs(e_g / np.array(e_o) - 1.0))))
        eng.close()
    print(json.dumps(dict(error_vs_oracle=out, case="C1", steps=steps)))


def run(args, env_extra, limit):
    env = dict(os.environ, **env_extra)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        print(json.dumps(dict(stopped=args, returncode=r.returncode)))
        sys.exit(1)    # a failed, faulted or timed-out child: nothing more on the GPU
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="C3,C1")
    ap.add_argument("--error", action="store_true")
    ap.add_argument("--child", nargs=2)
    ap.add_argument("--error-child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]))
    if a.error_child:
        return error_child()
    res = {}
    for case in a.cases.split(","):
        for rnd in range(a.rounds):
            order = list(VARIANTS) if rnd % 2 == 0 else list(reversed(VARIANTS))
            for name in order:
                kind, env = VARIANTS[name]
                r = run(["--child", case, str(kind)], env, 300)
                print(json.dumps(dict(round=rnd, variant=name, **r)), flush=True)
                res.setdefault(case, {}).setdefault(name, []).append(r["ms"])
    for case, d in res.items():
        summary = {k: statistics.median(v) for k, v in d.items()}
        summary["k1_over_k0_2pass"] = summary["k1"] / summary["k0-2pass"]
        print(json.dumps(dict(summary=case, ms_per_step=summary)), flush=True)
    if a.error:
        print(json.dumps(run(["--error-child"], {}, 600)), flush=True)


if __name__ == "__main__":
    main()
