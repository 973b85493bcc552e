"""The slot-packed bootstrapping entry points (CPU): OrionHipPackMonomials,
OrionHipUnpackMonomials, OrionHipSlotTraceNew and OrionHipBootstrapMany are
declared in include/orion_hip.h with these signatures, exported by the built
liborion_hip.so, bound in backend.SIGNATURES with their argument types, named
in INTEGRATION.md and wrapped by HipLibrary; the first three are capturable,
flushing calls in deferral.h's table, and OrionHipBootstrapMany, like
Bootstrap, has no row.  The two kernels' launchers are declared once, in
launch.h."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = {
    "OrionHipPackMonomials": r"int\s+ct\s*,\s*int\s+g",
    "OrionHipUnpackMonomials": r"int\s+ct\s*,\s*int\s+g\s*,\s*int\s+B",
    "OrionHipSlotTraceNew": r"int\s+ct\s*,\s*int\s+slots\s*,\s*int\s+mean",
    "OrionHipBootstrapMany": r"int\s+ct\s*,\s*int\s+slots",
}
WRAPPERS = {
    "pack_monomials": ["self", "ct", "g"],
    "unpack_monomials": ["self", "ct", "g", "batch"],
    "slot_trace_new": ["self", "ct", "slots", "mean"],
    "bootstrap_many": ["self", "ct", "slots"],
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


@pytest.fixture(scope="module")
def built_lib():
    from orion_amd import build
    return build.build()


@pytest.mark.parametrize("name", sorted(DECL))
def test_declared_in_header(name):
    assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, DECL[name]), _read("include", "orion_hip.h"))


@pytest.mark.parametrize("name", sorted(DECL))
def test_exported_by_library(built_lib, name):
    import ctypes
    import torch  # noqa: F401  (torch's HIP runtime first: one runtime per process, backend.load_library)
    assert getattr(ctypes.CDLL(built_lib), name)  # AttributeError: not exported


def test_bound_in_signatures():
    from orion_amd import backend
    i = backend.c_int
    want = {"OrionHipPackMonomials": [i, i], "OrionHipUnpackMonomials": [i, i, i], "OrionHipSlotTraceNew": [i, i, i],
            "OrionHipBootstrapMany": [i, i]}
    for name, args in want.items():
        assert name in backend.SIGNATURES, name
        got, res = backend.SIGNATURES[name]
        assert got == args and res is backend.c_int, name
        assert name not in backend.LATTIGO_SYMBOLS


@pytest.mark.parametrize("name", sorted(DECL))
def test_named_in_integration_doc(name):
    assert name in _read("INTEGRATION.md")


def test_python_wrappers_exist():
    import inspect
    from orion_amd.backend import HipLibrary
    for name, params in WRAPPERS.items():
        assert list(inspect.signature(getattr(HipLibrary, name)).parameters) == params, name
    assert inspect.signature(HipLibrary.slot_trace_new).parameters["mean"].default is False


def test_deferral_rows():
    text = _read("orion_amd", "csrc", "deferral.h")
    for name in ("OrionHipPackMonomials", "OrionHipUnpackMonomials", "OrionHipSlotTraceNew"):
        m = re.search(r'\{"%s",\s*(\d),\s*(\d)\}' % name, text)
        assert m and (m.group(1), m.group(2)) == ("1", "0"), name
    assert '"OrionHipBootstrapMany"' not in text and '"Bootstrap"' not in text


def test_launchers_declared_once():
    text = _read("orion_amd", "csrc", "launch.h")
    for name in ("orion_launch_mono_pack", "orion_launch_mono_unpack"):
        assert len(re.findall(r"\bint\s+%s\s*\(" % name, text)) == 1, name
        assert len(re.findall(r"\bint\s+%s\s*\(" % name, _read("orion_amd", "csrc", "kernels.hip"))) == 1, name
        assert not re.search(r"\bint\s+%s\s*\(" % name, _read("orion_amd", "csrc", "backend.hip")), name
