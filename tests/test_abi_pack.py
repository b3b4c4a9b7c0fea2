"""CPU: the entry points of the device-side event encoder (sw_set_event_class, sw_get_event_class, sw_pack_bound,
sw_pack_events[_device], sw_sync_pull_validated, sw_get_pack_stats) are exported by the library, listed in _lib.SIGNATURES
with as many arguments as the header declares; the ABI version is unchanged (symbols were only added); a NULL context is
refused before anything touches a device."""
import ctypes as C
import os
import re

from conftest import ROOT

NEW = ("sw_set_event_class", "sw_get_event_class", "sw_pack_bound", "sw_pack_events_device", "sw_pack_events",
       "sw_sync_pull_validated", "sw_get_pack_stats")


def test_symbols_signatures_and_version(pkg):
    L = pkg._lib.load()
    header = open(os.path.join(ROOT, "include", "swirld_hip.h")).read()
    for name in NEW:
        assert name in pkg._lib.SIGNATURES and hasattr(L, name), name
        m = re.search(r"\bint\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(pkg._lib.SIGNATURES[name][1]), name
    assert L.sw_version() == 7


def test_null_context_is_refused(pkg):
    L = pkg._lib.load()
    n = C.c_int64(-1)
    buf = C.create_string_buffer(256)
    assert L.sw_set_event_class(None, b"swirld", b"Event") == -22
    assert L.sw_get_event_class(None, buf, buf) == -22
    assert L.sw_pack_bound(None, 1, 0, C.byref(n), C.byref(n)) == -22
    assert L.sw_pack_events_device(None, 1, *([None] * 8), 0, *([None] * 3), 0, None, None, 0, None, None) == -22
    assert L.sw_pack_events(None, 1, *([None] * 8), 0, *([None] * 3), 0, None, None, 0, None, C.byref(n), C.byref(n)) == -22
    assert L.sw_sync_pull_validated(None, 0, None, 0, C.byref(n), C.byref(n), C.byref(n)) == -22
    assert L.sw_get_pack_stats(None, None, None, None, None) == -22
    assert n.value == -1


def test_front_end_methods(pkg):
    for name in ("set_event_class", "event_class", "pack_bound", "pack_events", "pack_events_device", "pack_stats", "pull_from"):
        assert callable(getattr(pkg.Hashgraph, name)), name
    import inspect
    assert inspect.signature(pkg.Hashgraph.pull_from).parameters["validate"].default is False
    assert callable(pkg.Node._is_plain)
