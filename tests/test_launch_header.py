"""Kernel-interface contract (CPU): the host launchers and the element-wise op
codes are declared once, in orion_amd/csrc/launch.h, and every file that
defines a launcher includes that header, so a signature or an op code that
drifts between the kernels and their caller does not compile."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orion_amd", "csrc")
# a declaration or a definition: the return type at the start of a line, the
# name, the parameter list (no parentheses inside), then `;` or `{`
FUNC = re.compile(r"^int\s+(orion_launch_\w+|orion_ntt_init)\s*\(([^()]*)\)\s*([;{])", re.M)


def _sources():
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".h", ".hip", ".cpp")):
            with open(os.path.join(CSRC, f)) as fh:
                out[f] = fh.read()
    return out


def test_launchers_are_declared_in_launch_h_only():
    src = _sources()
    protos = {f: [m.group(1) for m in FUNC.finditer(s) if m.group(3) == ";"] for f, s in src.items()}
    defs = {f: [m.group(1) for m in FUNC.finditer(s) if m.group(3) == "{"] for f, s in src.items()}
    assert [f for f, p in protos.items() if p] == ["launch.h"], protos
    defined = sorted(n for d in defs.values() for n in d)
    assert len(defined) > 20 and len(set(defined)) == len(defined)
    assert sorted(protos["launch.h"]) == defined  # each launcher declared once, none declared and missing
    # every call site's name is one of them (the pattern above misses no launcher)
    called = set(re.findall(r"\b(orion_launch_\w+|orion_ntt_init)\s*\(", "".join(src.values())))
    assert called == set(defined)


def test_op_codes_are_defined_once():
    holders = [f for f, s in _sources().items() if re.search(r"\benum\b[^;{]*\{[^}]*\bEW_ADD\b", s)]
    assert holders == ["launch.h"]


def test_every_file_that_defines_a_launcher_includes_launch_h():
    src = _sources()
    definers = [f for f, s in src.items() if any(m.group(3) == "{" for m in FUNC.finditer(s))]
    assert len(definers) >= 5
    for f in definers:
        assert re.search(r'^#include "launch\.h"', src[f], re.M), f
    assert re.search(r'^#include "launch\.h"', src["backend.hip"], re.M)
