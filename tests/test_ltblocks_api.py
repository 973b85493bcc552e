"""Blocked linear transform entry points (CPU): the three OrionHip*Blocks
symbols are declared in include/orion_hip.h, exported by the built
liborion_hip.so, bound in backend.SIGNATURES, named in INTEGRATION.md and
wrapped by HipLibrary and OrionStream; the evaluation is a capturable call in
deferral.h's table; the plan limits are the same in the kernel header and in
the planner's stand-alone check."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("OrionHipNewLinearTransformBlocks", "OrionHipEvaluateLinearTransformBlocks",
         "OrionHipDeleteLinearTransformBlocks")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


@pytest.fixture(scope="module")
def built_lib():
    from orion_amd import build
    return build.build()


@pytest.mark.parametrize("name", NAMES)
def test_declared_in_header(name):
    assert re.search(r"\b(int|void)\s+%s\s*\(" % name, _read("include", "orion_hip.h"))


@pytest.mark.parametrize("name", NAMES)
def test_exported_by_library(built_lib, name):
    import ctypes
    import torch  # noqa: F401  (torch's HIP runtime first: one runtime per process, backend.load_library)
    assert getattr(ctypes.CDLL(built_lib), name)  # AttributeError: not exported


@pytest.mark.parametrize("name", NAMES)
def test_bound_in_signatures(name):
    from orion_amd import backend
    assert name in backend.SIGNATURES
    assert backend.SIGNATURES[name][1] is (None if "Delete" in name else backend.c_int)
    assert name not in backend.LATTIGO_SYMBOLS


@pytest.mark.parametrize("name", NAMES)
def test_named_in_integration_doc(name):
    assert name in _read("INTEGRATION.md")


def test_python_wrappers_exist():
    import inspect
    from orion_amd import replay
    from orion_amd.backend import HipLibrary
    assert callable(HipLibrary.new_linear_transform_blocks)
    assert callable(HipLibrary.evaluate_linear_transform_blocks)
    assert callable(HipLibrary.delete_linear_transform_blocks)
    assert inspect.signature(HipLibrary.evaluate_linear_transform_blocks).parameters["rescale"].default is True
    assert callable(replay.block_groups)
    assert inspect.signature(replay.OrionStream.forward).parameters["blocked"].default is False


def test_evaluation_is_a_capturable_flushing_call():
    m = re.search(r'\{"OrionHipEvaluateLinearTransformBlocks",\s*(\d),\s*(\d)\}', _read("orion_amd", "csrc", "deferral.h"))
    assert m and (m.group(1), m.group(2)) == ("1", "0")
    assert "OrionHipNewLinearTransformBlocks" not in _read("orion_amd", "csrc", "deferral.h")  # no capture


def test_plan_limits_match_kernel_header():
    hdr, chk = _read("orion_amd", "csrc", "common.h"), _read("tests", "cpu", "lt_blocks_check.cpp")
    for name, short in (("LT_MAXB", "MAXB"), ("LT_MAXG", "MAXG"), ("LT_MAXSLOT", "MAXSLOT")):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, hdr)
        assert m and re.search(r"\b%s = %s\b" % (short, m.group(1)), chk), name
