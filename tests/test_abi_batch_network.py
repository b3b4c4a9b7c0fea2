"""CPU: the entry points of the gossip networks of a batch (sw_network_batch_*, sw_get_network_event_numbers,
sw_export_network_event_numbers[_device], sw_synth_schedule) are declared in the header, exported by the library and listed
in _lib.SIGNATURES with as many arguments as the header declares; none of them is named sw_batch_* or sw_export_batch_*
(tests/test_abi_batch.py and tests/test_abi_batch_export.py pin those families); the ABI version is unchanged (symbols were
only added); a NULL batch is refused before anything touches a device; the header documents the calls, the limits and the
one deviation; the front end has the methods; the kernel files are build dependencies, included in order."""
import ctypes as C
import importlib
import os
import re

import numpy as np

from conftest import ROOT

ARITY = {"sw_network_batch_begin": 5, "sw_network_batch_turns": 7, "sw_network_batch_run": 3, "sw_network_batch_get": 2,
         "sw_network_batch_heads": 2, "sw_network_batch_stats": 2, "sw_get_network_event_numbers": 5,
         "sw_export_network_event_numbers": 7, "sw_export_network_event_numbers_device": 8, "sw_synth_schedule": 6}


def header_text():
    return open(os.path.join(ROOT, "include", "swirld_hip.h")).read()


def test_every_prototype_has_its_signature_and_symbol(pkg):
    L = pkg._lib.load()
    protos = dict(re.findall(r"^int\s+(sw_\w+)\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S), flags=re.M))
    for name, arity in ARITY.items():
        assert name in protos, name
        assert len(protos[name].split(",")) == arity == len(pkg._lib.SIGNATURES[name][1]), name
        assert hasattr(L, name), name
        assert not name.startswith("sw_batch_") and not name.startswith("sw_export_batch_")
    assert sorted(k for k in pkg._lib.SIGNATURES if "network" in k or k == "sw_synth_schedule") == sorted(ARITY)
    assert "void* user_stream" in protos["sw_export_network_event_numbers_device"]
    assert L.sw_version() == 7


def test_header_documents_the_calls_the_limits_and_the_deviation(pkg):
    header = header_text()
    comments = " ".join(re.findall(r"/\*.*?\*/", header, flags=re.S))
    for name in ("sw_network_batch_begin", "sw_network_batch_turns", "sw_network_batch_run", "sw_network_batch_get", "sw_network_batch_heads",
                 "sw_network_batch_stats", "sw_get_network_event_numbers"):
        assert re.search(r"\* %s\s" % name, comments), "%s has no entry in the header's comment blocks" % name
    for word in ("NETWORK EVENT NUMBER", "no forks", "no crypto", "one turn at a time", "SW_NETWORK_STAGE_BROKEN", "swirld.py:135", "swirld.py:154-159",
                 "prefix-stable", "align64(128 G) + align64(16 B) + 2 B align64(4 cap_events)", "sw_synth_schedule"):
        assert word in comments, word
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(SW_NETWORK_\w+)\s+(\d+)", plain)}
    assert consts == dict(SW_NETWORK_BATCH_WORDS=6, SW_NETWORK_STAGE_BROKEN=4)
    assert len(pkg.engine.BatchNetworkStatus._fields) == consts["SW_NETWORK_BATCH_WORDS"]
    dev = open(os.path.join(ROOT, "py-swirld_amd", "csrc", "batch_network.hip.h")).read()
    assert re.search(r"STAGE_BROKEN = 4", dev)
    m = re.search(r"MAX_TURNS_PER_LAUNCH = (\d+);", dev)
    assert m and ("One launch per %s turns" % m.group(1)) in comments


def test_null_batch_is_refused(pkg):
    L = pkg._lib.load()
    n, off = C.c_int64(-7), (C.c_int64 * 2)(-7, -7)
    assert L.sw_network_batch_begin(None, None, None, None, None) == -22
    assert L.sw_network_batch_turns(None, None, None, None, None, None, C.byref(n)) == -22
    assert L.sw_network_batch_run(None, None, C.byref(n)) == -22
    assert L.sw_network_batch_get(None, None) == -22 and L.sw_network_batch_heads(None, None) == -22
    assert L.sw_network_batch_stats(None, (C.c_int64 * 4)()) == -22
    assert L.sw_get_network_event_numbers(None, 0, 0, 0, None) == -22
    assert L.sw_export_network_event_numbers(None, None, None, 0, off, None, C.byref(n)) == -22
    assert L.sw_export_network_event_numbers_device(None, None, None, 0, off, None, C.byref(n), None) == -22
    assert n.value == -7 and list(off) == [-7, -7]


def test_synth_schedule_needs_no_device(pkg):
    a, b = pkg.synth_schedule(5, 3, 0, 1000)
    assert a.dtype == b.dtype == np.int32 and (a != b).all() and set(a) == set(b) == set(range(5))
    for bad in ((1, 0, 0, 4), (3, 0, -1, 4), (3, 0, 0, -1)):
        try:
            pkg.synth_schedule(*bad)
        except pkg.SwirldHipError as e:
            assert e.code == -22
        else:
            raise AssertionError(bad)


def test_front_end(pkg):
    for name in ("network_begin", "network_turns", "network_run", "network_status", "network_heads", "event_numbers", "export_event_numbers",
                 "export_event_numbers_device", "network_stats"):
        assert callable(getattr(pkg.HashgraphBatch, name)), name
    assert pkg.engine.BatchNetworkStats._fields == ("calls", "turns", "imported", "launches")
    assert "synth_schedule" in pkg.__all__
    build = importlib.import_module("py-swirld_amd.build")
    assert "batch_network.hip.h" in build.DEPS and "batch_network_api.hip.h" in build.DEPS
    main = open(os.path.join(build.CSRC, "swirld_hip.hip")).read()
    assert main.index('#include "batch_export_api.hip.h"') < main.index('#include "batch_network_api.hip.h"')
    assert main.index('#include "batch_network.hip.h"') < main.index('#include "batch_api.hip.h"')
