"""The host-only deferral rule (orion_amd/csrc/deferral.h), checked on the CPU:
tests/cpu/deferral_check.cpp includes nothing else.  It compares the state
machine against op-by-op execution over every short call sequence, makes every
flush fail once, and runs the recorded forward streams of the reference
frontend (tests/golden/*_trace.json) through the state machine."""
import json
import os
import re
import subprocess

import pytest

from orion_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TRACES = ["lola_n15", "lola_n13", "mlp_n13", "mlp_n14", "resnet20_n13"]

# a rotation read again, or its source written first, runs on its own
_X = [{"op": "RotateNew", "args": [2, 4], "ret": 1}, {"op": "AddCiphertext", "args": [2, 1], "ret": 2},
      {"op": "AddCiphertext", "args": [3, 1], "ret": 3}, {"op": "DeleteCiphertext", "args": [1], "ret": None}]
HAND = {"read_again": _X, "fused": _X[:2] + _X[3:], "unread": [_X[0], _X[3]]}


def forward(name):
    with open(os.path.join(GOLD, f"{name}_trace.json")) as f:
        return [e for e in json.load(f)["events"] if e["phase"] == "forward"]


def lines(name, events):
    """one call per line: op, its first two arguments, the handle it returned (-1: none)"""
    def num(v):
        return v if isinstance(v, int) and not isinstance(v, bool) and 0 <= v < 2 ** 31 else -1
    out = [f"stream {name}"]
    for e in events:
        a = (list(e["args"]) + [None, None])[:2]
        out.append(f"{e['op']} {num(a[0])} {num(a[1])} {num(e['ret'])}")
    return out


@pytest.fixture(scope="module")
def check():
    """compiles and runs the program once: its output, and the counts of each stream"""
    os.makedirs(hipbuild.BUILD, exist_ok=True)
    exe = os.path.join(hipbuild.BUILD, "deferral_check")
    txt = os.path.join(hipbuild.BUILD, "deferral_streams.txt")
    streams = {name: forward(name) for name in TRACES}
    streams.update(HAND)
    with open(txt, "w") as fh:
        for name, ev in streams.items():
            fh.write("\n".join(lines(name, ev)) + "\n")
    # host code only, compiled as build.py compiles hostmath.cpp (no offload arch)
    cc = subprocess.run([hipbuild.HIPCC, "-O2", "-std=c++17", "-Wall", "-I", hipbuild.CSRC,
                         os.path.join(ROOT, "tests", "cpu", "deferral_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe, txt], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    counts = {}
    for m in re.finditer(r"^stream (\S+): rotations fused (\d+) dropped (\d+) plain (\d+); "
                         r"moddowns merged (\d+) plain (\d+) dropped (\d+)$", run.stdout, re.M):
        counts[m.group(1)] = tuple(int(g) for g in m.groups()[1:])
    assert set(counts) == set(streams), run.stdout
    return run.stdout, counts


def test_deferral_state_machine(check):
    """Observationally equivalent to the op-by-op calls over every sequence of
    at most 4 calls from every pending state, and every failed flush poisons
    exactly the handles reported as written."""
    out, _ = check
    m = re.search(r"^(\d+) call sequences of length <= 4 equivalent", out, re.M)
    assert m and int(m.group(1)) > 1000000, out
    m = re.search(r"^(\d+) failed flushes poisoned what they owed", out, re.M)
    assert m and int(m.group(1)) > 1000, out


@pytest.mark.parametrize("name,fused", [("lola_n15", 10), ("lola_n13", "all"), ("mlp_n13", None),
                                        ("mlp_n14", None), ("resnet20_n13", None)])
def test_reference_stream_hits_deferred_rotate_add(check, name, fused):
    """The frontend's own calls (the recorded stream as the fork issues it,
    debug Decrypt/Decode included) reach the library's deferred rotate-and-add
    for every `out += out.roll(k)` of LoLA (linear.py:72-73): RotateNew,
    AddCiphertext into its source, DeleteCiphertext of the rotation -- so the
    op-by-op replay the bench times runs them as one key switch each."""
    _, counts = check
    f, d, p = counts[name][:3]
    n_rot = sum(e["op"] == "RotateNew" for e in forward(name))
    assert f + d + p == n_rot
    if fused == "all":
        fused = n_rot
    if fused is not None:
        assert f == fused and p == 0
    assert counts["read_again"][:3] == (0, 0, 1)
    assert counts["fused"][:3] == (1, 0, 0)
    assert counts["unread"][:3] == (0, 1, 0)


def test_reference_stream_merges_moddown_and_rescale(check):
    """Five times per LoLA pass a ModDown is followed by the rescale of its
    result as the very next call ("one division by P q_l"): each
    pair reaches the merged form, where the launch sizes allow it."""
    _, counts = check
    merged, plain, dropped = counts["lola_n15"][3:]
    assert merged == 5
    assert merged + plain + dropped == sum(e["op"] in ("EvaluateLinearTransform", "MulRelinCiphertextNew")
                                           for e in forward("lola_n15"))
