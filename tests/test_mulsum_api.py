"""The sum-of-products entry point (CPU): OrionHipMulRelinSum is declared in
include/orion_hip.h, exported by the built liborion_hip.so, bound in
backend.SIGNATURES with its argument types, named in INTEGRATION.md and wrapped
by HipLibrary; it is a capturable, flushing call in deferral.h's table."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "OrionHipMulRelinSum"


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


@pytest.fixture(scope="module")
def built_lib():
    from orion_amd import build
    return build.build()


def test_declared_in_header():
    assert re.search(r"\bint\s+%s\s*\(\s*const\s+int\s*\*\s*a\s*,\s*const\s+int\s*\*\s*b\s*,\s*int\s+n\s*\)\s*;" % NAME,
                     _read("include", "orion_hip.h"))


def test_exported_by_library(built_lib):
    import ctypes
    import torch  # noqa: F401  (torch's HIP runtime first: one runtime per process, backend.load_library)
    assert getattr(ctypes.CDLL(built_lib), NAME)  # AttributeError: not exported


def test_bound_in_signatures():
    from orion_amd import backend
    assert NAME in backend.SIGNATURES
    args, res = backend.SIGNATURES[NAME]
    assert args == [backend.P(backend.c_int), backend.P(backend.c_int), backend.c_int] and res is backend.c_int
    assert NAME not in backend.LATTIGO_SYMBOLS


def test_named_in_integration_doc():
    assert NAME in _read("INTEGRATION.md")


def test_python_wrapper_exists():
    import inspect
    from orion_amd.backend import HipLibrary
    assert list(inspect.signature(HipLibrary.mul_relin_sum).parameters) == ["self", "a_handles", "b_handles"]


def test_call_is_capturable_and_flushes():
    m = re.search(r'\{"%s",\s*(\d),\s*(\d)\}' % NAME, _read("orion_amd", "csrc", "deferral.h"))
    assert m and (m.group(1), m.group(2)) == ("1", "0")
