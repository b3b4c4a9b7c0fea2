"""CPU: the entry points of device-side event creation (sw_set_signing_keys, sw_clear_signing_keys, sw_get_signing_members,
sw_sign_events[_device], sw_create_events[_device], sw_get_sign_stats) are exported by the library, listed in
_lib.SIGNATURES with as many arguments as the header declares; the ABI version is unchanged (symbols were only added); a
NULL context is refused before anything touches a device."""
import ctypes as C
import os
import re

from conftest import ROOT

NEW = ("sw_set_signing_keys", "sw_clear_signing_keys", "sw_get_signing_members", "sw_sign_events_device", "sw_sign_events",
       "sw_create_events_device", "sw_create_events", "sw_get_sign_stats")


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
    assert L.sw_set_signing_keys(None, 1, None, None) == -22
    assert L.sw_clear_signing_keys(None) == -22
    assert L.sw_get_signing_members(None, None) == -22
    assert L.sw_sign_events_device(None, 1, *([None] * 6), 0, *([None] * 7)) == -22
    assert L.sw_sign_events(None, 1, *([None] * 6), 0, *([None] * 6)) == -22
    assert L.sw_create_events_device(None, 1, *([None] * 6), 0, None, None, C.byref(n), None, None) == -22
    assert L.sw_create_events(None, 1, *([None] * 6), 0, None, C.byref(n), None, None) == -22
    assert L.sw_get_sign_stats(None, None, None, None, None, None) == -22
    assert n.value == -1


def test_front_end_methods(pkg):
    for name in ("set_signing_seeds", "clear_signing_seeds", "signing_members", "sign_events", "sign_events_device", "create_events",
                 "create_events_device", "sign_stats"):
        assert callable(getattr(pkg.Hashgraph, name)), name
