"""Bootstrapping-key entry points (CPU): the OrionHip* calls that prepare,
count, describe, export and import a bootstrapper's key records are declared
in include/orion_hip.h, exported by the built liborion_hip.so, bound in
backend.SIGNATURES (and are no Lattigo symbols) and named in INTEGRATION.md;
the Python wrappers and the OrionStream helpers exist."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> C return type
NAMES = {
    "OrionHipBootstrapPrepareKeys": "int",
    "OrionHipBootstrapMissingKeys": "int",
    "OrionHipBootstrapKeyCount": "int",
    "OrionHipBootstrapKeyBytes": "unsigned long",
    "OrionHipBootstrapKeyInfo": "int",
    "OrionHipExportBootstrapKey": "int",
    "OrionHipImportBootstrapKey": "int",
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


@pytest.fixture(scope="module")
def built_lib():
    from orion_amd import build
    return build.build()


@pytest.mark.parametrize("name", sorted(NAMES))
def test_declared_in_header(name):
    ret = NAMES[name].replace(" ", r"\s+")
    assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), _read("include", "orion_hip.h"))


@pytest.mark.parametrize("name", sorted(NAMES))
def test_exported_by_library(built_lib, name):
    import ctypes
    import torch  # noqa: F401  (torch's HIP runtime first: one runtime per process, backend.load_library)
    assert getattr(ctypes.CDLL(built_lib), name)  # AttributeError: not exported


@pytest.mark.parametrize("name", sorted(NAMES))
def test_bound_in_signatures(name):
    from orion_amd import backend
    assert name in backend.SIGNATURES
    want = backend.c_ulong if NAMES[name] == "unsigned long" else backend.c_int
    assert backend.SIGNATURES[name][1] is want
    assert name not in backend.LATTIGO_SYMBOLS


@pytest.mark.parametrize("name", sorted(NAMES))
def test_named_in_integration_doc(name):
    assert name in _read("INTEGRATION.md")


def test_python_wrappers_exist():
    from orion_amd import dist
    from orion_amd.backend import HipLibrary
    from orion_amd.replay import OrionStream
    for fn in ("bootstrap_prepare_keys", "bootstrap_missing_keys", "bootstrap_key_info", "export_bootstrap_key",
               "import_bootstrap_key"):
        assert callable(getattr(HipLibrary, fn)), fn
    for fn in ("bootstrap_slot_counts", "export_bootstrap_keys", "import_bootstrap_keys"):
        assert callable(getattr(OrionStream, fn)), fn
    assert callable(dist.broadcast_bootstrap_keys)


def test_slot_counts_come_from_the_trace():
    """bootstrap_slot_counts() reads the NewBootstrapper events of the trace
    (no scheme is made: the stream object is built without its constructor)."""
    import json
    from orion_amd.replay import GOLDEN, OrionStream
    for name in ("resnet20_n13", "lola_n13"):
        with open(os.path.join(GOLDEN, name + "_trace.json")) as fh:
            events = json.load(fh)["events"]
        st = OrionStream.__new__(OrionStream)
        st._events = events
        want = []
        for ev in events:
            if ev["op"] == "NewBootstrapper" and ev["args"][1] not in want:
                want.append(ev["args"][1])
        assert st.bootstrap_slot_counts() == want
        assert bool(want) == (name == "resnet20_n13")
