"""Writes tests/golden/ref_hotpath_<case>.npz: the stages of tests/ref_hotpath.py as the reference's own modules compute
them (oracle/_ref/libpic1dp_ref_<case>_small.so, built by `make -C oracle ref` where the reference tree lies), for the
small variant of every case of oracle/ref_cases.json.  Data the reference writes while it runs; no program text.

    python tests/golden/gen_ref_hotpath.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle  # noqa: E402
import ref_hotpath  # noqa: E402


def main():
    oracle.build()
    for case in oracle.ref_case_names():
        if not case.endswith("_small"):
            continue
        rec = ref_hotpath.record(oracle.Ref.get(case))
        path = ref_hotpath.fixture_path(case[:-len("_small")])
        np.savez_compressed(path, **rec)
        print("%s: %d arrays, %d bytes" % (os.path.basename(path), len(rec), os.path.getsize(path)))


if __name__ == "__main__":
    main()
