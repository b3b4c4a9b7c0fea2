"""CPU: the export entry points (sw_get_known_heights_device, sw_export_payload[_device], sw_sync_pull,
sw_get_export_stats) are exported by the library, listed in _lib.SIGNATURES and declared in the header; the ABI version
is unchanged (symbols were only added); a NULL context is refused before anything touches a device."""
import ctypes as C
import os
import re

from conftest import ROOT

NEW = ("sw_get_known_heights_device", "sw_export_payload_device", "sw_export_payload", "sw_sync_pull", "sw_get_export_stats")


def test_symbols_signatures_and_version(pkg):
    L = pkg._lib.load()
    header = open(os.path.join(ROOT, "include", "swirld_hip.h")).read()
    for name in NEW:
        assert name in pkg._lib.SIGNATURES and hasattr(L, name)
        assert re.search(r"\bint\s+%s\(" % name, header), name
    assert L.sw_version() == 7


def test_null_context_is_refused(pkg):
    L = pkg._lib.load()
    n = C.c_int64(-1)
    assert L.sw_get_known_heights_device(None, 0, None, None) == -22
    assert L.sw_export_payload_device(None, 0, None, 0, *([None] * 8), None, C.byref(n)) == -22
    assert L.sw_export_payload(None, 0, None, 0, *([None] * 8), C.byref(n)) == -22
    assert L.sw_sync_pull(None, 0, None, 0, C.byref(n), C.byref(n)) == -22
    assert L.sw_get_export_stats(None, None, None, None) == -22
    assert n.value == -1


def test_front_end_methods(pkg):
    for name in ("known_heights_device", "export_payload_device", "export_size", "export_payload", "pull_from", "export_stats"):
        assert callable(getattr(pkg.Hashgraph, name)), name
