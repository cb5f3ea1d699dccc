"""tests/golden/step_launches.json: what every scenario of tests/test_gpu_step_launches.py launches, recorded from the
library as built -- run on a GPU with the library whose behaviour is to be pinned (round 27: the parent of the commit that
moved the step path's decisions into step_plan.cpp); the test then holds every later library to it.
    python tests/golden/gen_step_launches.py [out.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

if __name__ == "__main__":
    import pic1dp_amd
    import test_gpu_step_launches as t
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "step_launches.json")
    table = {}
    for name in t.SCENARIOS:      # (the two-species scenario last: written after every other one)
        table[name] = t.observe(pic1dp_amd, os.environ.__setitem__, lambda k: os.environ.pop(k, None), name)
        print(name, json.dumps(table[name]), flush=True)
        with open(out, "w") as f:
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in table.items()) + "\n}\n")
    print(out, len(table), "scenarios")
