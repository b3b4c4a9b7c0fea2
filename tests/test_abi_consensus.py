"""CPU: the entry points for round received and consensus timestamp (sw_get_round_received, sw_get_consensus_time,
sw_export_ordered[_device], sw_get_consensus_stats) are exported by the library, listed in _lib.SIGNATURES and declared in
the header; the ABI version is unchanged (symbols were only added); a NULL context is refused before anything touches a
device; the front end has the methods."""
import ctypes as C
import os
import re

from conftest import ROOT

NEW = ("sw_get_round_received", "sw_get_consensus_time", "sw_export_ordered_device", "sw_export_ordered", "sw_get_consensus_stats")


def test_symbols_signatures_and_version(pkg):
    L = pkg._lib.load()
    header = open(os.path.join(ROOT, "include", "swirld_hip.h")).read()
    for name in NEW:
        assert name in pkg._lib.SIGNATURES and hasattr(L, name)
        proto = re.search(r"\bint\s+%s\(([^;]*)\);" % name, header)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(pkg._lib.SIGNATURES[name][1]), name     # the arity of the ctypes entry
        assert re.search(r"%s\s.*swirld\.py:283-309" % name, header), "%s: its header entry names swirld.py:283-309" % name
    assert L.sw_version() == 7


def test_null_context_is_refused(pkg):
    L = pkg._lib.load()
    n = C.c_int64(-1)
    out = (C.c_int32 * 4)(9, 9, 9, 9)
    assert L.sw_get_round_received(None, 0, 4, out) == -22
    assert L.sw_get_consensus_time(None, 0, 4, out) == -22
    assert L.sw_export_ordered_device(None, 0, 0, *([None] * 5), None) == -22
    assert L.sw_export_ordered(None, 0, 4, out, *([None] * 4)) == -22
    assert L.sw_get_consensus_stats(None, C.byref(n), C.byref(n), C.byref(n), C.byref(n)) == -22
    assert n.value == -1 and list(out) == [9, 9, 9, 9]


def test_front_end_methods(pkg):
    for name in ("round_received", "consensus_time", "export_ordered", "export_ordered_device", "consensus_stats"):
        assert callable(getattr(pkg.Hashgraph, name)), name
    from collections.abc import Mapping
    assert issubclass(pkg.node._ConsensusView, Mapping)
