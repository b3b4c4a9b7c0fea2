"""CPU: the entry points of the wire form of a sync answer (sw_pack_message_bound, sw_pack_message[_device],
sw_unpack_message[_device], sw_export_message[_device], sw_ingest_message[_device], sw_get_wire_stats) are exported by the
library, listed in _lib.SIGNATURES with as many arguments as the header declares; the ABI version is unchanged (symbols were
only added); a NULL context is refused before anything touches a device; the front end has the methods and Node the switch,
off."""
import ctypes as C
import os
import re

from conftest import ROOT

NEW = ("sw_pack_message_bound", "sw_pack_message_device", "sw_pack_message", "sw_unpack_message_device", "sw_unpack_message",
       "sw_export_message_device", "sw_export_message", "sw_ingest_message_device", "sw_ingest_message", "sw_get_wire_stats")


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
    n = C.c_int64(-7)
    for name in NEW:
        args = [None if a is pkg._lib.SIGNATURES[name][1][0] or a is C.c_void_p or a is C.c_char_p else
                C.byref(n) if a is C.POINTER(C.c_int64) else 0 for a in pkg._lib.SIGNATURES[name][1]]
        assert getattr(L, name)(*args) == -22, name
    assert n.value == -7


def test_front_end_methods_and_the_switch(pkg):
    for name in ("pack_message_bound", "pack_message", "pack_message_device", "unpack_message", "unpack_message_device", "export_message",
                 "export_message_device", "ingest_message", "ingest_message_device", "wire_stats"):
        assert callable(getattr(pkg.Hashgraph, name)), name
    assert pkg.Node.device_wire is False
    assert pkg.node.WIRE_PREFIX == b"\x80\x04\x8c\x12py-swirld_amd.node\x8c\x05Event\x93\x940\x8e"
