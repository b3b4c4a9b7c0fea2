"""CPU: the entry points of the gossip turn (sw_create_event, sw_gossip_turn, sw_get_turn_stats) are exported by the
library and listed in _lib.SIGNATURES with as many arguments as the header declares; the header documents them; the flag
and stage constants and the result struct agree between header and Python; the ABI version is unchanged (symbols were only
added); a NULL context is refused before anything touches a device."""
import ctypes as C
import os
import re

from conftest import ROOT

NEW = ("sw_create_event", "sw_gossip_turn", "sw_get_turn_stats")
CONSTANTS = ("SW_TURN_VALIDATE", "SW_TURN_DATA", "SW_TURN_TRUNKS", "SW_TURN_NO_CONSENSUS", "SW_TURN_STAGE_NONE", "SW_TURN_STAGE_PULLED",
             "SW_TURN_STAGE_CREATED", "SW_TURN_STAGE_DIVIDED", "SW_TURN_STAGE_FAME", "SW_TURN_STAGE_ORDERED")


def header_text():
    return open(os.path.join(ROOT, "include", "swirld_hip.h")).read()


def test_symbols_signatures_and_version(pkg):
    L = pkg._lib.load()
    header = header_text()
    for name in NEW:
        assert name in pkg._lib.SIGNATURES and hasattr(L, name), name
        m = re.search(r"\bint\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(pkg._lib.SIGNATURES[name][1]), name
    assert L.sw_version() == 7


def test_header_documents_the_calls():
    header = header_text()
    comments = " ".join(re.findall(r"/\*.*?\*/", header, flags=re.S))
    for name in NEW:
        assert re.search(r"\* %s\s" % name, comments), "%s has no entry in the header's comment blocks" % name
    for word in ("DEFINED BY EQUIVALENCE", "sw_sync_pull_walk(dst, dst_head, src, src_head", "wall_clock64", "swirld.py:86", "swirld.py:87"):
        assert word in comments, word


def test_constants_and_result_struct_agree(pkg):
    header = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    for name in CONSTANTS:
        m = re.search(r"#define\s+%s\s+(\d+)" % name, header)
        assert m, name
        assert int(m.group(1)) == getattr(pkg._lib, name), name
    flags = [getattr(pkg._lib, k) for k in CONSTANTS[:4]]
    assert sorted(flags) == [1, 2, 4, 8]
    body = re.search(r"typedef struct sw_turn_result \{(.*?)\} sw_turn_result;", header, flags=re.S).group(1)
    fields = []
    for decl in re.findall(r"int64_t\s+([^;]+);", body):
        fields += [f.strip() for f in decl.split(",")]
    assert fields == [k for k, _ in pkg._lib.TurnResult._fields_]
    assert all(t is C.c_int64 for _, t in pkg._lib.TurnResult._fields_) and C.sizeof(pkg._lib.TurnResult) == 8 * len(fields)
    assert pkg.engine.TurnResult._fields == tuple(fields) + ("new_rounds",)


def test_null_context_is_refused(pkg):
    L = pkg._lib.load()
    n = C.c_int64(-1)
    res = pkg._lib.TurnResult()
    assert L.sw_create_event(None, 0, -1, -1, 0.0, None, -1, C.byref(n), None, None) == -22
    assert L.sw_gossip_turn(None, 0, 0, None, 0, 0.0, None, -1, 0, None, 0, C.byref(res), C.sizeof(res)) == -22
    assert L.sw_get_turn_stats(None, None, None, None, None, None, None) == -22
    assert n.value == -1


def test_front_end(pkg):
    for name in ("create_event", "gossip_turn", "turn_stats"):
        assert callable(getattr(pkg.Hashgraph, name)), name
    for name in ("turn", "run", "partner", "head", "event_ids", "round", "transactions", "round_received", "consensus_time", "ordered_data"):
        assert callable(getattr(pkg.DeviceNetwork, name)), name
    import inspect
    sig = inspect.signature(pkg.Hashgraph.gossip_turn)
    assert list(sig.parameters)[1:7] == ["peer", "member", "my_head", "peer_head", "t", "data"]
    assert {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY} == dict(validate=True, data_store=False, trunks=False, consensus=True)
