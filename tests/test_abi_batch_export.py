"""CPU: the whole-batch exports (sw_export_batch_*) are declared in the header, exported by the library and listed in
_lib.SIGNATURES with as many arguments as the header declares; none of them is named sw_batch_* (tests/test_abi_batch.py pins
that family); the ABI version is unchanged (symbols were only added); a NULL batch is refused before anything touches a
device; the front end has the methods; the kernel file is a build dependency."""
import ctypes as C
import importlib
import os
import re

from conftest import ROOT

NAMES = ["sw_export_batch_ordered", "sw_export_batch_new_rounds", "sw_export_batch_events", "sw_export_batch_rounds"]


def declared():
    header = open(os.path.join(ROOT, "include", "swirld_hip.h")).read()
    return dict(re.findall(r"^int\s+(sw_export_batch_\w+)\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.M))


def test_every_prototype_has_its_signature_and_symbol(pkg):
    L = pkg._lib.load()
    protos = declared()
    assert sorted(protos) == sorted(NAMES + [nm + "_device" for nm in NAMES] + ["sw_export_batch_stats"])
    for name, args in protos.items():
        assert not name.startswith("sw_batch_")
        assert name in pkg._lib.SIGNATURES and hasattr(L, name), name
        assert len(args.split(",")) == len(pkg._lib.SIGNATURES[name][1]), name
    for nm in NAMES:   # the device twin: the same arguments and the stream
        assert protos[nm + "_device"].count(",") == protos[nm].count(",") + 1 and "void* user_stream" in protos[nm + "_device"]
    assert sorted(k for k in pkg._lib.SIGNATURES if k.startswith("sw_export_batch_")) == sorted(protos)
    assert L.sw_version() == 7


def test_header_documents_the_calls():
    header = open(os.path.join(ROOT, "include", "swirld_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", header, flags=re.S))
    for name in NAMES + ["sw_export_batch_stats"]:
        assert re.search(r"\* %s\s" % name, comments), "%s has no entry in the header's comment blocks" % name
    for word in ("RAGGED", "SIZING", "HOST memory", "16-byte", "FROZEN", "size and retry"):
        assert word in comments, word


def test_null_batch_is_refused(pkg):
    L = pkg._lib.load()
    off, total = (C.c_int64 * 2)(-7, -7), C.c_int64(-7)
    assert L.sw_export_batch_ordered(None, None, None, 0, off, None, None, None, C.byref(total)) == -22
    assert L.sw_export_batch_ordered_device(None, None, None, 0, off, None, None, None, C.byref(total), None) == -22
    assert L.sw_export_batch_new_rounds(None, None, 0, off, None, C.byref(total)) == -22
    assert L.sw_export_batch_new_rounds_device(None, None, 0, off, None, C.byref(total), None) == -22
    assert L.sw_export_batch_events(None, None, None, 0, off, None, None, None, None, C.byref(total)) == -22
    assert L.sw_export_batch_events_device(None, None, None, 0, off, None, None, None, None, C.byref(total), None) == -22
    assert L.sw_export_batch_rounds(None, None, None, 0, off, None, None, None, C.byref(total)) == -22
    assert L.sw_export_batch_rounds_device(None, None, None, 0, off, None, None, None, C.byref(total), None) == -22
    assert L.sw_export_batch_stats(None, (C.c_int64 * 4)()) == -22
    assert list(off) == [-7, -7] and total.value == -7


def test_front_end(pkg):
    for name in ("export_ordered", "export_new_rounds", "export_events", "export_rounds", "export_ordered_device", "export_new_rounds_device",
                 "export_events_device", "export_rounds_device", "step_arrays", "export_stats"):
        assert callable(getattr(pkg.HashgraphBatch, name)), name
    assert pkg.engine.BatchStepArrays._fields == ("took", "rounds_off", "rounds", "tx_off", "event", "round_received", "time", "n_failed")
    build = importlib.import_module("py-swirld_amd.build")
    assert "batch_export.hip.h" in build.DEPS
    assert all(os.path.exists(os.path.join(build.CSRC, d)) for d in build.DEPS)
    main = open(os.path.join(build.CSRC, "swirld_hip.hip")).read()
    assert main.index('#include "batch_api.hip.h"') < main.index('#include "batch_export.hip.h"')
