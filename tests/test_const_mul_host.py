"""x / lx in two operations: the host's decision procedure (pic1dp_amd/csrc/const_mul.cpp) against the division itself.
No GPU: tests/const_mul_check.cpp is a program of its own, built with the host sanitizers."""
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_operation_quotient_is_decided_exactly_and_equals_the_division(tmp_path):
    """For lx in {2 pi / 0.36, 4 pi, 1, 17, 0.1, 3 * 2^-7} the procedure decides whether fma(yh, x, RN(yl x)) is RN(x / lx)
    for every double x; where proven, 10^8 random operands in [0, lx], every double within 2 ulp of the cell boundaries of
    nx = 2, 192, 1024, 8192 and the procedure's own worst cases are compared bit for bit.  A constant the procedure rejects
    (a literal found by search) has an operand that really differs, and its context takes the five operations.  Built with
    const_mul.cpp and hostcheck.cpp under AddressSanitizer and UndefinedBehaviorSanitizer (host code only), with the
    product's floating-point flags."""
    spec = importlib.util.spec_from_file_location("pic1dp_amd_build", os.path.join(ROOT, "pic1dp_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    csrc = os.path.join(ROOT, "pic1dp_amd", "csrc")
    exe = str(tmp_path / "const_mul_check")
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-x", "hip", "--offload-host-only", "-O3", "-g", "-std=c++17",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "const_mul_check.cpp")] +
                          [os.path.join(csrc, f) for f in ("const_mul.cpp", "hostcheck.cpp")] + ["-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("6 constants proven, ") and last.endswith(", 0 differ"), r.stdout
    compared = int(last.split(", ")[1].split()[0])
    assert compared >= 6 * 10**8, last
    assert "lx 0x1.800000000019fp+3: NOT proven" in r.stdout and "context: five operations" in r.stdout, r.stdout
