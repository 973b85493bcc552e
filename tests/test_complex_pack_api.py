"""The complex-packing entry points (CPU): OrionHipConjugateNew,
OrionHipPackComplex, OrionHipUnpackComplex and OrionHipBootstrapPacked are
declared in include/orion_hip.h with these signatures, exported by the built
liborion_hip.so, bound in backend.SIGNATURES with their argument types, named
in INTEGRATION.md and wrapped by HipLibrary; the first three are capturable,
flushing calls in deferral.h's table, and OrionHipBootstrapPacked, like
Bootstrap, has no row."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = {
    "OrionHipConjugateNew": r"int\s+ct",
    "OrionHipPackComplex": r"int\s+a\s*,\s*int\s+b",
    "OrionHipUnpackComplex": r"int\s+ct\s*,\s*int\s*\*\s*out2",
    "OrionHipBootstrapPacked": r"int\s+ct\s*,\s*int\s+slots",
}
WRAPPERS = {
    "conjugate_new": ["self", "ct"],
    "pack_complex": ["self", "a", "b"],
    "unpack_complex": ["self", "ct"],
    "bootstrap_packed": ["self", "ct", "slots"],
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
    i, pi = backend.c_int, backend.P(backend.c_int)
    want = {"OrionHipConjugateNew": [i], "OrionHipPackComplex": [i, i], "OrionHipUnpackComplex": [i, pi],
            "OrionHipBootstrapPacked": [i, i]}
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


def test_deferral_rows():
    text = _read("orion_amd", "csrc", "deferral.h")
    for name in ("OrionHipConjugateNew", "OrionHipPackComplex", "OrionHipUnpackComplex"):
        m = re.search(r'\{"%s",\s*(\d),\s*(\d)\}' % name, text)
        assert m and (m.group(1), m.group(2)) == ("1", "0"), name
    assert '"OrionHipBootstrapPacked"' not in text and '"Bootstrap"' not in text
