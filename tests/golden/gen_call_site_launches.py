"""tests/golden/call_site_launches.json: what every call of every scenario of tests/test_gpu_call_site_launches.py launches,
recorded from the library as built -- run on a GPU with the library whose behaviour is to be pinned (round 31: the parent of
the commit that moved the call sites' decisions into call_plan.cpp); the test then holds every later library to it.
    python tests/golden/gen_call_site_launches.py [out.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

if __name__ == "__main__":
    import pic1dp_amd
    import test_gpu_call_site_launches as t
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "call_site_launches.json")
    pool, table = [], {}
    for name in t.SCENARIOS:
        calls = t.encoded(t.observe(pic1dp_amd, os.environ.__setitem__, lambda k: os.environ.pop(k, None), name), pool)
        first = calls if not table else first
        table[name] = t.written(calls, None if not table else first)
        print(name, len(calls), "calls", flush=True)
        with open(out, "w") as f:
            f.write('{"bytes": [\n' + ",\n".join(json.dumps(b, separators=(",", ":")) for b in pool) + '\n],\n"scenarios": {\n' +
                    ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in table.items()) + "\n}}\n")
    print(out, len(table), "scenarios")
