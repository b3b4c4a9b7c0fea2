"""CPU: the kernels of csrc/exact_history.hip.h run thread by thread on the host, and the vote flush of exact.hip.h with
one lane (tests/exact_history_emul.cpp, a stand-alone program built with AddressSanitizer and UBSan; every case checks
itself against a std::map or a plain loop and exits nonzero on the first difference):
    grow       an initial capacity of 4 entries — growth and reindex several times — overwrites of existing keys, colliding
               hashes, first-insertion order of the log, the look-up kernel on stored, absent and out-of-range pairs;
    overflow   a ceiling of 24 entries: the sticky overflow word, nothing stored behind it, nothing written out of bounds;
    expand n   the row / bitmask table expanded into entries behind entries the log already holds: empty rows, bits in the
               last partial word (n = 5, 65, 130), the row offsets by the three phases of the one-workgroup scan with 1024
               and with 7 threads;
    tables     normalise, defaults and record of the per-event tables, zero produced items included.
The host side of the library (checks, growth, streams) is NOT covered here: tests/test_gpu_exact_history.py does that."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("exact_history_emul") / "exact_history_emul")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "exact_history_emul.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("case", [("grow",), ("overflow",), ("expand", "5"), ("expand", "65"), ("expand", "130"), ("tables",)],
                         ids=lambda c: "-".join(c))
def test_case(emul, case):
    r = subprocess.run([emul] + list(case), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
