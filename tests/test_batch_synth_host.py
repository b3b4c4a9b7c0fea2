"""CPU: the batch's device generator (csrc/batch_synth.hip.h, swbs::begin / swbs::generate) through
tests/batch_synth_main.cpp, a stand-alone program built with AddressSanitizer and UBSan and linked with csrc/synth.cpp.  The
program runs the very statements k_batch_synth runs, over allocations of exactly their size, and compares creators, parents,
heights, timestamps, signatures and per-event defaults with sw_synth_hashgraph bit for bit: 8 member counts (2 to 70, with
the clique of one member of mode 1 at 3 members) x 10 parameter sets (the four modes and p0 = 0 / p0 = 1 in modes 1 to 3)
x N = n, n + 1, 600 x one call or instalments of n, 1, 7, 0, 64, 65, ... events with dropped (refused) calls in between."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("batch_synth") / "batch_synth_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "batch_synth_main.cpp"), os.path.join(ROOT, "py-swirld_amd", "csrc", "synth.cpp"), "-o", exe])
    return exe


def test_generator_equals_the_host_function_bit_for_bit(prog):
    r = subprocess.run([prog], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    word, runs, events = r.stdout.split()
    assert word == "ok" and int(runs) == 8 * 10 * 3 * 2
    # every run stores N events: N = n, n + 1 and 600 for each member count, 10 parameter sets, twice
    assert int(events) == 20 * sum(2 * n + 1 + 600 for n in (2, 3, 4, 5, 16, 33, 64, 70))


def test_python_layer_has_the_entry_points():
    """The ctypes table and HashgraphBatch carry the four functions (the header side: tests/test_abi.py)."""
    import importlib
    lib = importlib.import_module("py-swirld_amd._lib")
    eng = importlib.import_module("py-swirld_amd.engine")
    arity = {"sw_synth_batch_begin": 6, "sw_synth_batch": 3, "sw_synth_batch_stats": 2, "sw_get_batch_events": 9}
    for name, n_args in arity.items():
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == n_args, name
    for method in ("synth_begin", "synth", "synth_stats", "events"):
        assert callable(getattr(eng.HashgraphBatch, method)), method
