"""The cases of tests/test_gpu_trims_bitwise.py and the generator of its golden file.

    python tests/gen_trims_digests.py           (on a GPU, from a build of the commit whose bits are to be held:
                                                 tests/golden/trims_digests.json was recorded from the parent of the
                                                 change that shortened locate and folded the unit charge, through
                                                 PIC1DP_LIB=<a build of that commit>)

With the exact charge sum (set_charge_sum(1)) a run is bit-reproducible; the digests of the marker state after 1, 2 and 20
steps, through step() and through the sub-steps, are the record."""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "trims_digests.json")

# 2 pi / 0.36 (the default box), 4 pi, and a box length for which the two-operation x / lx is NOT proven
# (tests/const_mul_check.cpp): its context divides in five operations
LX = {"default": 2.0 * math.pi / 0.36, "4pi": 4.0 * math.pi, "unproven": float.fromhex("0x1.800000000019fp+3")}
SHAPES = {
    # odd count, one kept mode; a unit species of charge -1: the unit instances with the charge folded
    "one": dict(nparticle_max=200_001, nx=64),
    # two species of charge -1 and +1 (the second of mass 4: the power-of-two instances beside the unit ones)
    "two": dict(nparticle_max=65_537, nx=8, nspecies=2, species_charge=[-1.0, 1.0], species_mass=[1.0, 4.0],
                species_temperature=[1.0, 1.0], species_temperature2=[1.0, 1.0], species_density=[0.9, 0.9], species_v0=[5.0, 5.0]),
    # a unit species of charge -2: the charge must NOT be folded
    "z2": dict(nparticle_max=65_537, nx=8, species_charge=[-2.0]),
}
STEPS = (1, 2, 20)
PATHS = ("step", "substeps")
CASES = [(shape, lx) for shape in SHAPES for lx in LX]


def run_case(amd, shape, lx, path):
    """the digests [[x, v, w, p] per species] after 1, 2 and 20 steps"""
    e = amd.Pic1dp(amd.make_input(lx=LX[lx], **SHAPES[shape]))
    try:
        e.particle_load()
        e.set_charge_sum(1)
        e.interaction_collect_charge()
        e.field_solve_electric()
        out, done = [], 0
        for n in STEPS:
            if path == "step":
                e.step(n - done)
            else:
                for _ in range(n - done):
                    e.substep(1)
                    e.substep(2)
            done = n
            out.append([[int(v) for v in row] for row in e.state_digest()])
        return out
    finally:
        e.close()


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    import pic1dp_amd as amd
    rec = {"steps": list(STEPS), "lx": {k: float(v).hex() for k, v in LX.items()}, "digests": {}}
    for shape, lx in CASES:
        for path in PATHS:
            rec["digests"]["%s/%s/%s" % (shape, lx, path)] = run_case(amd, shape, lx, path)
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d records" % (out, len(rec["digests"])))


if __name__ == "__main__":
    main()
