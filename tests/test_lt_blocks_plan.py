"""The blocked linear transform's host-only pieces, checked on the CPU.

The layout planner (orion_amd/csrc/lt_blocks.h): tests/cpu/lt_blocks_check.cpp
includes nothing else and asserts anchor cases derived by hand.  The replay's
grouping (orion_amd.replay.block_groups): a pure function over a stream's
events, run on the recorded ResNet-20 and LoLA streams."""
import json
import os
import re
import subprocess

import pytest

from orion_amd import build as hipbuild
from orion_amd.replay import block_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIPPED = ("Decrypt", "Decode", "DeletePlaintext")


def test_lt_blocks_planner():
    os.makedirs(hipbuild.BUILD, exist_ok=True)
    exe = os.path.join(hipbuild.BUILD, "lt_blocks_check")
    # host code only, compiled as build.py compiles hostmath.cpp (no offload arch)
    cc = subprocess.run([hipbuild.HIPCC, "-O1", "-std=c++17", "-Wall", "-I", hipbuild.CSRC,
                         os.path.join(ROOT, "tests", "cpu", "lt_blocks_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all anchor cases hold" in run.stdout, run.stdout


def _events(name):
    with open(os.path.join(ROOT, "tests", "golden", f"{name}_trace.json")) as fh:
        return json.load(fh)["events"]


@pytest.fixture(scope="module")
def resnet():
    ev = _events("resnet20_n13")
    return ev, [e for e in ev if e["phase"] == "forward"], block_groups(ev)


def test_every_four_input_convolution_is_found_as_4x4(resnet):
    ev, fwd, groups = resnet
    by_start = {g["start"]: g for g in groups}
    four = [g for g in groups if g["cols"] == 4]
    # read off the stream independently: with the deletes and the debug
    # decryptions left out, a row over four inputs is L L A L A L A R
    letters = {"EvaluateLinearTransform": "L", "AddCiphertextNew": "A", "RescaleNew": "R"}
    ops = "".join(letters.get(e["op"], "x") for e in fwd
                  if e["op"] not in SKIPPED and e["op"] != "DeleteCiphertext")
    rows4 = len(re.findall(r"(?<![LA])LLALALAR", ops))
    runs44 = len(re.findall(r"(?<![LAR])(?:LLALALAR){4}(?!L)", ops))
    assert rows4 > 0 and sum(g["rows"] for g in four) == rows4
    assert runs44 > 0 and sum(1 for g in four if g["rows"] == 4) == runs44
    lt_events = [i for i, e in enumerate(fwd) if e["op"] == "EvaluateLinearTransform"]
    covered = {i for g in groups for i in g["skip"]}
    assert set(lt_events) <= covered  # every transform of the pass belongs to a group
    for g in four:
        if g["rows"] != 4:
            continue
        ops = "".join({"EvaluateLinearTransform": "L", "AddCiphertextNew": "A", "DeleteCiphertext": "d",
                       "RescaleNew": "R"}.get(fwd[i]["op"], "?") for i in range(g["start"], g["end"] + 1))
        assert ops.count("L") == 16 and ops.count("A") == 12 and ops.count("R") == 4 and "?" not in ops
        assert ops.startswith("LLAdLdAdLdAdRd")
        assert len({t for row in g["lts"] for t in row}) == 16 and len(set(g["cts"])) == 4
        for i, row in enumerate(g["lts"]):  # T[i][j] is the transform applied to ct[j] in row i
            for j, t in enumerate(row):
                assert any(fwd[k]["op"] == "EvaluateLinearTransform" and fwd[k]["args"] == [t, g["cts"][j]]
                           for k in g["skip"])
    first = min(four, key=lambda g: g["start"])
    assert (first["start"], first["end"], first["rows"]) == (106, 163, 4) and by_start[106] is first


def test_lola_has_only_single_blocks():
    groups = block_groups(_events("lola_n15"))
    assert groups and all((g["rows"], g["cols"]) == (1, 1) for g in groups)


def _live_after(fwd, groups):
    """trace ids alive after the pass; with groups, each blocked layer's events
    are replaced as OrionStream.forward(blocked=True) replaces them"""
    acts = {}
    for g in groups:
        if g["rows"] * g["cols"] == 1:
            continue
        for fi in g["skip"]:
            acts[fi] = "skip"
        for fi, _ in g["outs"]:
            acts[fi] = "out"
    live = {0}  # the input
    for fi, e in enumerate(fwd):
        if e["op"] in SKIPPED or acts.get(fi) == "skip":
            continue
        if e["op"] == "DeleteCiphertext":
            assert e["args"][0] in live, (fi, e)  # a delete that is replayed finds its handle
            live.discard(e["args"][0])
        elif e["ret"] is not None:
            if acts.get(fi) is None:  # a replayed op reads a live ciphertext (an "out" only binds a row)
                assert e["args"][1 if e["op"] == "EvaluateLinearTransform" else 0] in live, (fi, e)
            live.add(e["ret"])
    return live


def test_grouped_bookkeeping_leaves_the_same_live_handles(resnet):
    ev, fwd, groups = resnet
    assert any(g["rows"] * g["cols"] > 1 for g in groups)
    assert _live_after(fwd, groups) == _live_after(fwd, [])
    # no event belongs to two groups, and each group's outputs are its rows' rescales
    seen = set()
    for g in groups:
        assert not (seen & set(g["skip"]))
        seen |= set(g["skip"])
        assert len(g["outs"]) == g["rows"] == len(g["lts"]) and all(len(r) == g["cols"] for r in g["lts"])
        assert all(fwd[fi]["op"] == "RescaleNew" and fwd[fi]["ret"] == rid for fi, rid in g["outs"])
