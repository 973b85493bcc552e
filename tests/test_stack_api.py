"""Stack / slice entry points (CPU): OrionHipStackCiphertexts and
OrionHipSliceCiphertext are declared in include/orion_hip.h, exported by the
built liborion_hip.so, bound in backend.SIGNATURES and named in
INTEGRATION.md; the gather kernel's table size is the same in the kernel
header and in the Python module."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("OrionHipStackCiphertexts", "OrionHipSliceCiphertext")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


@pytest.fixture(scope="module")
def built_lib():
    from orion_amd import build
    return build.build()


@pytest.mark.parametrize("name", NAMES)
def test_declared_in_header(name):
    assert re.search(r"\bint\s+%s\s*\(" % name, _read("include", "orion_hip.h"))


@pytest.mark.parametrize("name", NAMES)
def test_exported_by_library(built_lib, name):
    import ctypes
    import torch  # noqa: F401  (torch's HIP runtime first: one runtime per process, backend.load_library)
    assert getattr(ctypes.CDLL(built_lib), name)  # AttributeError: not exported


@pytest.mark.parametrize("name", NAMES)
def test_bound_in_signatures(name):
    from orion_amd import backend
    assert name in backend.SIGNATURES
    assert backend.SIGNATURES[name][1] is backend.c_int
    assert name not in backend.LATTIGO_SYMBOLS


@pytest.mark.parametrize("name", NAMES)
def test_named_in_integration_doc(name):
    assert name in _read("INTEGRATION.md")


def test_python_wrappers_exist():
    from orion_amd.backend import HipLibrary
    from orion_amd.replay import OrionStream
    assert callable(HipLibrary.stack_ciphertexts) and callable(HipLibrary.slice_ciphertext)
    assert callable(OrionStream.encrypt_images) and callable(OrionStream.forward_stacked)


def test_table_size_constant_matches_kernel_header():
    from orion_amd import backend
    m = re.search(r"#define\s+ORION_MAXGATHER\s+(\d+)", _read("orion_amd", "csrc", "common.h"))
    assert m and int(m.group(1)) == backend.STACK_TABLE_SIZE
