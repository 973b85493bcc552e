"""The host side of the hoisted rotations (orion_amd/csrc/hoist.h and HoistRoute
of ntt_route.h), checked on the CPU: tests/cpu/hoist_check.cpp includes nothing
else.  Over every n in 1..64 the keys-per-launch chunks cover 0..n-1 exactly
once, in order, none over ORION_MAXHOIST; the register bound on the digit count
is monotone; the routes of the GPU tests' shapes have one decomposition and
their outputs' ModDowns carry the automorphism.  The program is built with the
address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

from orion_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    with open(os.path.join(hipbuild.CSRC, "hoist.h")) as fh:
        m = re.search(rf"#define\s+{name}\s+(\d+)", fh.read())
    assert m, name
    return int(m.group(1))


def test_hoist_chunks_bound_and_routes():
    os.makedirs(hipbuild.BUILD, exist_ok=True)
    exe = os.path.join(hipbuild.BUILD, "hoist_check")
    # host code only, compiled as build.py compiles hostmath.cpp (no offload arch)
    cc = subprocess.run([hipbuild.HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host",
                         "-fsanitize=address,undefined", "-I", hipbuild.CSRC,
                         os.path.join(ROOT, "tests", "cpu", "hoist_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"hoist plan holds: (\d+) chunks, register bound (\d+), (\d+) routes", run.stdout)
    assert m, run.stdout
    per = _define("ORION_MAXHOIST")
    assert int(m.group(1)) == sum(-(-n // per) for n in range(1, 65))
    # the bound the GPU tests read off the header is the one the rule applies
    assert int(m.group(2)) == _define("ORION_HOIST_MAXBETA")
    assert int(m.group(3)) >= 2 * 30


def test_limits_are_what_the_documents_say():
    with open(os.path.join(ROOT, "include", "orion_hip.h")) as fh:
        hdr = fh.read()
    assert "up to %d keys" % _define("ORION_MAXHOIST") in hdr
    with open(os.path.join(hipbuild.CSRC, "common.h")) as fh:
        group = int(re.search(r"#define\s+ORION_MAXGROUP\s+(\d+)", fh.read()).group(1))
    assert "1 <= n <= %d" % group in hdr
