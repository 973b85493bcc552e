"""The host side of a sum of ciphertext products (orion_amd/csrc/tensor_sum.h),
checked on the CPU: tests/cpu/tensor_sum_check.cpp includes nothing else.  It
compares the header's lazy accumulation and rare Barrett reductions with
unsigned __int128 arithmetic on primes of 40, 46, 50, 52, 55, 60 and 61 bits
(all residues q - 1, all 0, 10^4 random tuples per prime and pair count, in the
header's own order and in the kernel's), and asserts the chunk planner's launch
counts and the documented accumulation bounds."""
import os
import re
import subprocess

from orion_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tensor_sum_arithmetic_and_planner():
    os.makedirs(hipbuild.BUILD, exist_ok=True)
    exe = os.path.join(hipbuild.BUILD, "tensor_sum_check")
    # host code only, compiled as build.py compiles hostmath.cpp (no offload arch)
    cc = subprocess.run([hipbuild.HIPCC, "-O1", "-std=c++17", "-Wall", "-I", hipbuild.CSRC,
                         os.path.join(ROOT, "tests", "cpu", "tensor_sum_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"tensor sums agree with 128-bit arithmetic on (\d+) tuples; the planner and the bounds hold",
                  run.stdout)
    # 14 primes x 8 pair counts x (10^4 random + 3 planted) tuples
    assert m and int(m.group(1)) >= 14 * 8 * 10003, run.stdout


def test_pairs_per_launch_is_what_the_documents_say():
    with open(os.path.join(hipbuild.CSRC, "tensor_sum.h")) as fh:
        m = re.search(r"#define\s+ORION_MAXTSUM\s+(\d+)", fh.read())
    assert m
    with open(os.path.join(ROOT, "include", "orion_hip.h")) as fh:
        assert "ceil(n / %s) launches" % m.group(1) in fh.read()
