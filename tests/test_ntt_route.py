"""The host-only launch planner (orion_amd/csrc/ntt_route.h), checked on the
CPU: tests/cpu/ntt_route_check.cpp includes nothing else, asserts anchor cases
derived from the rules as written, and reproduces every decision commit
a9bb9bd's predicates made over the grid recorded in
tests/golden/ntt_routes.json."""
import base64
import hashlib
import json
import os
import subprocess
import zlib

from orion_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ntt_route_planner():
    with open(os.path.join(ROOT, "tests", "golden", "ntt_routes.json")) as fh:
        doc = json.load(fh)
    table = zlib.decompress(base64.b64decode(doc["table_zlib_b64"]))
    assert doc["commit"] == "a9bb9bd"
    assert hashlib.sha256(table).hexdigest() == doc["sha256"]
    assert table.count(b"\n") == doc["lines"]
    os.makedirs(hipbuild.BUILD, exist_ok=True)
    exe = os.path.join(hipbuild.BUILD, "ntt_route_check")
    txt = os.path.join(hipbuild.BUILD, "ntt_routes.txt")
    with open(txt, "wb") as fh:
        fh.write(table)
    # host code only, compiled as build.py compiles hostmath.cpp (no offload arch)
    cc = subprocess.run([hipbuild.HIPCC, "-O1", "-std=c++17", "-Wall", "-I", hipbuild.CSRC,
                         os.path.join(ROOT, "tests", "cpu", "ntt_route_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe, txt], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "%d recorded decisions reproduced" % doc["decisions"] in run.stdout, run.stdout
