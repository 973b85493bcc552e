"""The hoisted-rotation entry points (CPU): OrionHipRotateHoisted and
OrionHipRotateSum are declared in include/orion_hip.h, exported by the built
liborion_hip.so, bound in backend.SIGNATURES with their argument types, named
in INTEGRATION.md and wrapped by HipLibrary; they are capturable, flushing
calls in deferral.h's table."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = {
    "OrionHipRotateHoisted": r"\(\s*int\s+ct\s*,\s*const\s+int\s*\*\s*amounts\s*,\s*int\s+n\s*,\s*int\s*\*\s*out\s*\)",
    "OrionHipRotateSum": r"\(\s*int\s+ct\s*,\s*const\s+int\s*\*\s*amounts\s*,\s*int\s+n\s*\)",
}
NAMES = sorted(DECL)


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


@pytest.fixture(scope="module")
def built_lib():
    from orion_amd import build
    return build.build()


@pytest.mark.parametrize("name", NAMES)
def test_declared_in_header(name):
    assert re.search(r"\bint\s+%s\s*%s\s*;" % (name, DECL[name]), _read("include", "orion_hip.h"))


@pytest.mark.parametrize("name", NAMES)
def test_exported_by_library(built_lib, name):
    import ctypes
    import torch  # noqa: F401  (torch's HIP runtime first: one runtime per process, backend.load_library)
    assert getattr(ctypes.CDLL(built_lib), name)  # AttributeError: not exported


def test_bound_in_signatures():
    from orion_amd import backend
    ip, i = backend.P(backend.c_int), backend.c_int
    want = {"OrionHipRotateHoisted": [i, ip, i, ip], "OrionHipRotateSum": [i, ip, i]}
    for name in NAMES:
        assert name in backend.SIGNATURES
        args, res = backend.SIGNATURES[name]
        assert args == want[name] and res is backend.c_int
        assert name not in backend.LATTIGO_SYMBOLS


@pytest.mark.parametrize("name", NAMES)
def test_named_in_integration_doc(name):
    assert name in _read("INTEGRATION.md")


def test_python_wrappers_exist():
    import inspect
    from orion_amd.backend import HipLibrary
    assert list(inspect.signature(HipLibrary.rotate_hoisted).parameters) == ["self", "ct", "amounts"]
    assert list(inspect.signature(HipLibrary.rotate_sum).parameters) == ["self", "ct", "amounts"]


@pytest.mark.parametrize("name", NAMES)
def test_call_is_capturable_and_flushes(name):
    m = re.search(r'\{"%s",\s*(\d),\s*(\d)\}' % name, _read("orion_amd", "csrc", "deferral.h"))
    assert m and (m.group(1), m.group(2)) == ("1", "0")
