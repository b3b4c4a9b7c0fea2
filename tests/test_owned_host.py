"""CPU: csrc/owned.h, the owning types of the context's device buffers, pinned buffers, events and streams, through
tests/owned_main.cpp (a stand-alone program built with AddressSanitizer and UBSan against a fake HIP runtime of its own: a
table of live handles).  Per type: the destructor frees, a moved-from object frees nothing, move-assignment over a live
object frees the old one; DBuf::release leaves the block live and uncounted, an aliased range is never freed;
Pinned::reserve does nothing at or below the capacity, frees before it allocates, and is empty after a failed allocation;
Event::ensure creates once.  The program itself fails on a double free, a free of an unknown handle, a handle live at exit,
and on any step after which the library's live-resource counts differ from the table's."""
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
    exe = str(tmp_path_factory.mktemp("owned") / "owned_main")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), os.path.join(ROOT, "tests", "owned_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("case", ["dbuf", "pinned", "event", "stream"])
def test_owning_type(prog, case):
    # (the program's own table of handles is the leak check)
    r = subprocess.run([prog, case], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split() == ["ok", case]
