#!/usr/bin/env python3
"""sweep_direction_probe.py -- would sweeping the markers back and forth let a step reuse the Infinity Cache?  The
ceiling, measured on the pure tiled 4-read / 3-write stream before any product kernel changes: launch pairs back to
back over ONE slab, forward -> forward against forward -> backward (mirrored 64-pair chunks), at the headline's size,
the 8-way share's and c2's, with three cache policies: non-temporal everywhere (the product's choice at these sizes),
plain everywhere, plain only within R bytes of marker state of either slab end, plain only in the first R bytes.

    python tools/sweep_direction_probe.py [rounds] [sizes] [R at either end, MiB] [R at the head alone, MiB]   (comma-separated lists)

Every (size, policy, pair) is timed `rounds` times, the rounds interleaved over the whole table, five trials of ten
launch pairs each; a line gives the median ms per launch over all its trials and their min - max spread, and the
last column of a forward -> backward line its median against the forward -> forward one of the same policy."""
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pic1dp_amd import probe as probe_lib  # noqa: E402  (libpic1dp_probe.so: measurement code, not the product)

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
sizes = [int(float(s)) for s in sys.argv[2].split(",")] if len(sys.argv) > 2 else [10**8, 12_500_000, 10**7]
MIB = 1 << 20
radii = [int(r) for r in sys.argv[3].split(",")] if len(sys.argv) > 3 else [64, 128, 192, 256]
heads = [int(r) for r in sys.argv[4].split(",")] if len(sys.argv) > 4 else [128, 256]
# (name, plain bytes, at the head alone)
policies = [("nt", 0, 0), ("plain", -1, 0)] + [("ends 2x%3d MiB" % r, r * MIB, 0) for r in radii] + [
    ("head %3d MiB" % r, r * MIB, 1) for r in heads]

times = {}
for rnd in range(rounds):
    for n in sizes:
        for name, plain_bytes, head_only in policies:
            for alt in (0, 1):
                times.setdefault((n, name, alt), []).extend(probe_lib.sweep(n, alt, plain_bytes, pairs=10, trials=5, head_only=head_only))

print("SWEEP markers     policy          pair                 median ms   min      max      GB/s   fb / ff")
for n in sizes:
    for name, _, _ in policies:
        ff = statistics.median(times[(n, name, 0)])
        for alt in (0, 1):
            t = times[(n, name, alt)]
            med = statistics.median(t)
            print("SWEEP %-11d %-15s %-20s %.4f    %.4f   %.4f   %5.0f  %s"
                  % (n, name, "forward -> backward" if alt else "forward -> forward", med, min(t), max(t),
                     56.0 * n / 1e6 / med, ("%.4f" % (med / ff)) if alt else ""), flush=True)
