"""CPU: the per-chunk function of the whole-batch export (csrc/batch_export.hip.h, swbx::export_chunk) through
tests/batch_export_main.cpp, a stand-alone program built with AddressSanitizer and UBSan.  The program runs the very function
the kernel runs over random ragged plans (1 to 3000 hashgraphs, empty runs at the front, in the middle and at the end, elements
of 1 / 4 / 8 bytes, rows of 4, 5, 33 and 64 columns at their strides) with every source segment, the offsets and the output in
allocations of exactly their size, and compares with a naive loop: a byte read or written out of bounds ends it."""
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
    exe = str(tmp_path_factory.mktemp("batch_export") / "batch_export_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "batch_export_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_plans_equal_the_naive_gather(prog, seed):
    r = subprocess.run([prog, str(seed), "40"], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    word, plans, entries = r.stdout.split()
    assert word == "ok" and int(plans) == 40 * 15 and int(entries) > 100000
