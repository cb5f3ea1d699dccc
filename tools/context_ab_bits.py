#!/usr/bin/env python3
"""context_ab_bits.py -- do two builds of libpic1dp_hip.so compute the same bits?  Each library runs every case TWICE, each
run in a process of its own (PIC1DP_LIB picks the library at import): 50 steps, then sha256 of fields, energy history and
downloaded markers.  A case only counts where the first library equals ITSELF between its two runs -- FP64 atomics of
several waves into one LDS cell come in no fixed order --, and there the second must equal it byte for byte.
    python tools/context_ab_bits.py --parent OLD.so --result NEW.so [--log FILE]
Cases: the default grid, nx 1024, two kept modes; each with one wave's worth of markers (128: 64 lanes x one pair, one
order of additions), and with kind 1 of the charge sum (integer accumulators: order-independent) at one workgroup's
worth (1536) and at the default marker count.  Exit status 1 if a deterministic case differs or none is deterministic."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = {"default": dict(), "nx1024": dict(nx=1024), "two_modes": dict(nmode=2, modes=[1, 2])}
MODES = {"one_wave": (128, 0), "exact_one_workgroup": (1536, 1), "exact_default_count": (0, 1)}   # markers (0: the input's), charge sum
KEYS = ("electric", "chargeden", "mode_re", "mode_im", "energy_history", "x", "v", "p", "w", "pred_kind")


def one(grid, mode):
    sys.path.insert(0, ROOT)
    import numpy as np

    import pic1dp_amd
    markers, charge_sum = MODES[mode]
    kw = dict(GRIDS[grid])
    if markers:
        kw["nparticle_max"] = markers
    e = pic1dp_amd.Pic1dp(pic1dp_amd.make_input(**kw), device=0)
    if charge_sum:
        e.set_charge_sum(charge_sum)
    e.particle_load()
    e.interaction_collect_charge()
    e.field_solve_electric()
    e.step(50)
    h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]
    out = {"pred_kind": e.predict_kind()}
    f = e.get_field()
    for k in ("electric", "chargeden", "mode_re", "mode_im"):
        out[k] = h(f[k])
    out["energy_history"] = h(e.energy_history())
    g = e.particles_download()
    for k in "xvpw":
        out[k] = h(g[k])
    e.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--result")
    ap.add_argument("--log")
    ap.add_argument("--one", nargs=2, metavar=("GRID", "MODE"))
    a = ap.parse_args()
    if a.one:
        return one(*a.one)
    log = open(a.log, "w") if a.log else None

    def say(line):
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    bad = deterministic = 0
    for mode in MODES:
        for grid in GRIDS:
            runs = {}
            for who, lib in (("parent", a.parent), ("result", a.result), ("parent again", a.parent), ("result again", a.result)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", grid, mode], capture_output=True, text=True,
                                   timeout=240, env=dict(os.environ, PIC1DP_LIB=os.path.abspath(lib)))
                if r.returncode != 0:     # (a fault, an abort, an error: nothing more is started)
                    say("## %s, %s, %s: exit status %d\n%s" % (grid, mode, who, r.returncode, r.stderr[-2000:]))
                    return 2
                runs[who] = json.loads(r.stdout.strip().splitlines()[-1])
            diff = lambda x, y: [k for k in KEYS if runs[x][k] != runs[y][k]]
            own, other = diff("parent", "parent again"), diff("result", "result again")
            cross = sorted(set(diff("parent", "result") + diff("parent again", "result again")))
            if own or other:
                say("## %s, %s: not deterministic -- parent against itself differs in %s, result against itself in %s; no verdict"
                    % (grid, mode, ",".join(own) or "nothing", ",".join(other) or "nothing"))
                continue
            deterministic += 1
            say("## %s, %s: each library equals itself; parent against result %s" % (grid, mode, "EQUAL as bytes in all of %s" % ",".join(KEYS)
                                                                                if not cross else "DIFFER in " + ",".join(cross)))
            bad += bool(cross)
    say("## verdict: %d deterministic cases, %d of them differ between parent and result" % (deterministic, bad))
    return 1 if bad or not deterministic else 0


if __name__ == "__main__":
    sys.exit(main())
