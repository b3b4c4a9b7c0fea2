"""CPU: the entry points of the batch (sw_batch_*) are exported by the library and listed in _lib.SIGNATURES with as many
arguments as the header declares; the header documents them; the stage constants and the width of a summary row agree between
header, device code and Python; the ABI version is unchanged (symbols were only added); sw_batch_bytes needs no device and
agrees with the layout header's formula; a NULL batch is refused before anything touches a device."""
import ctypes as C
import os
import re

from conftest import ROOT
from test_batch_layout_host import formula, up64


def header_text():
    return open(os.path.join(ROOT, "include", "swirld_hip.h")).read()


def declared(header):
    return re.findall(r"^(?:int|int64_t|const char\*)\s+(sw_batch_\w+)\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.M)


def test_every_prototype_has_its_signature_and_symbol(pkg):
    L = pkg._lib.load()
    protos = declared(header_text())
    names = [nm for nm, _ in protos]
    assert len(names) == len(set(names)) == 18
    for want in ("sw_batch_bytes", "sw_batch_create", "sw_batch_destroy", "sw_batch_last_error", "sw_batch_append", "sw_batch_step",
                 "sw_batch_get_summary", "sw_batch_get_transactions", "sw_batch_get_new_rounds", "sw_batch_get_witness_order"):
        assert want in names, want
    for name, args in protos:
        assert name in pkg._lib.SIGNATURES and hasattr(L, name), name
        assert len(args.split(",")) == len(pkg._lib.SIGNATURES[name][1]), name
    assert sorted(k for k in pkg._lib.SIGNATURES if k.startswith("sw_batch_")) == sorted(names)
    assert L.sw_version() == 7


def test_header_documents_the_calls_and_the_limits():
    header = header_text()
    comments = " ".join(re.findall(r"/\*.*?\*/", header, flags=re.S))
    for name in ("sw_batch_bytes", "sw_batch_create", "sw_batch_append", "sw_batch_step", "sw_batch_get_summary"):
        assert re.search(r"\* %s\s" % name, comments), "%s has no entry in the header's comment blocks" % name
    for word in ("swirld.py:325-328", "ATOMIC", "FROZEN", "fixed at create", "id index", "cap_events + 3"):
        assert word in comments, word


def test_constants_agree(pkg):
    header = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(SW_BATCH_\w+)\s+(\d+)", header)}
    assert consts == dict(SW_BATCH_SUMMARY_WORDS=9, SW_BATCH_STAGE_NONE=0, SW_BATCH_STAGE_DIVIDE=1, SW_BATCH_STAGE_FAME=2, SW_BATCH_STAGE_ORDER=3)
    assert len(pkg.engine.BatchSummary._fields) == consts["SW_BATCH_SUMMARY_WORDS"]
    assert pkg.engine.BATCH_STAGES == {0: None, 1: "divide", 2: "fame", 3: "order"}
    dev = open(os.path.join(ROOT, "py-swirld_amd", "csrc", "batch.hip.h")).read()
    assert re.search(r"STAGE_NONE = 0, STAGE_DIVIDE = 1, STAGE_FAME = 2, STAGE_ORDER = 3", dev)


def test_batch_bytes_without_a_device(pkg):
    need = pkg.HashgraphBatch.bytes_needed
    for B, n, E, R in ((1, 4, 40, 0), (10000, 4, 40, 0), (48, 8, 700, 0), (8, 70, 1600, 200), (2048, 64, 8192, 64), (8192, 64, 600, 40)):
        assert need(B, n, E, R) == up64(B * 512) + up64(B * 64) + B * formula(n, (n + 15) // 16 * 16, E, R), (B, n, E, R)
    assert need(2048, 64, 8192, 64) > 4 << 30
    assert 0 < need(1 << 24, 4, 1 << 20, 64) < 1 << 62
    # every argument inside its own range, the product beyond 64 bits: refused, not wrapped
    for bad in ((0, 4, 40, 0), (1, 0, 40, 0), (1, 1025, 40, 0), (1, 4, 0, 0), (1, 4, 40, -1), (8192, 1024, 1 << 30, 0), (1 << 24, 1024, 1 << 30, 1 << 30),
                (1 << 24, 64, 1 << 30, 64)):
        assert need(*bad) == -1, bad


def test_null_batch_is_refused(pkg):
    L = pkg._lib.load()
    n = C.c_int64(-7)
    assert L.sw_batch_destroy(None) == -22
    assert L.sw_batch_append(None, None, None, None, None, None, None) == -22
    assert L.sw_batch_step(None, None, C.byref(n)) == -22 and n.value == -7
    assert L.sw_batch_get_summary(None, None) == -22
    assert L.sw_batch_get_round(None, 0, 0, 0, None) == -22
    assert L.sw_batch_get_transactions(None, 0, 0, 0, None, None, None) == -22
    assert L.sw_batch_create(1, 4, None, 6, 40, 0, 0, None) == -22


def test_front_end(pkg):
    assert pkg.HashgraphBatch is pkg.engine.HashgraphBatch and "HashgraphBatch" in pkg.__all__
    for name in ("append", "step", "summary", "summary_array", "close", "heights", "rounds", "can_see", "witnesses", "witness_order", "famous",
                 "famous_events", "consensus", "new_rounds", "transactions", "ordered", "bytes_needed"):
        assert callable(getattr(pkg.HashgraphBatch, name)), name
    build = __import__("importlib").import_module("py-swirld_amd.build")
    assert "batch.hip.h" in build.DEPS and "batch_layout.h" in build.DEPS
