"""CPU: csrc/entry_plan.h, the host-side planning of the call forms, through tests/entry_plan_main.cpp (a stand-alone program
built with AddressSanitizer and UBSan).  first_misaligned over aligned rows, rows off by one and by half an alignment, NULL
and zero-byte rows, for alignments 4 / 8 / 16; and Stage against the literal Carve::take sequences it replaces in
sw_pack_events, sw_pack_message and sw_unpack_message: the same offsets and total, the copies in call order with their byte
counts, and a download sized after the launches copies that size."""
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
    exe = str(tmp_path_factory.mktemp("entry_plan") / "entry_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "entry_plan_main.cpp"), "-o", exe])
    return exe


def run(prog, *args):
    r = subprocess.run([prog, *map(str, args)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-3000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def test_first_misaligned(prog):
    got = {name: int(v) for name, v in run(prog, "align")}
    assert got == dict(aligned=-1, off_by_one_16=1, off_by_one_8=0, off_by_one_4=2, half_16=0, half_8=0, half_4=0, null_rows=-1,
                       zero_byte_rows=-1, skipped_then_bad=2, first_of_two=0, empty=-1)


def r256(b):
    return (b + 255) & ~255


def model(form, k, opt):
    """(room of every piece in call order, [(piece, upload bytes)], [(piece, download bytes before, after the late sizes)])."""
    db = 5 * k + 3 if opt else 0
    if form == "pack_events":
        bm, bw = 200 * k + db, 300 * k + db
        rooms = [k * 32, k * 32, k, k * 4, k * 8, k * 64, (k + 1) * 8 if opt else 0, db, k if opt else 0, (k + 1) * 8, (k + 1) * 8, bm, bw, k]
        ups = [(i, rooms[i]) for i in range(9)]
        downs = [(9, rooms[9], rooms[9]), (10, rooms[10], rooms[10]), (11, 0, 7 * k), (12, 0, 9 * k)] + ([(13, k, k)] if opt else [])
    elif form == "pack_message":
        bound = 100 + 250 * k + db
        rooms = [32, k * 32, k * 32, k * 32, k, k * 4, k * 8, k * 64, (k + 1) * 8 if opt else 0, db, k if opt else 0, 8, bound]
        ups = [(i, rooms[i]) for i in range(11)]
        downs = [(12, 0, 90 + 11 * k)]
    else:
        kk = k // 2
        rooms = [64 + 150 * k + db, 32, k * 32, k * 32, k * 32, k, k * 4, k * 8, k * 64, (k + 1) * 8, k, db + 16]
        ups = [(0, rooms[0])]
        late = [32, kk * 32, kk * 32, kk * 32, kk, kk * 4, kk * 8, kk * 64, (kk + 1) * 8, kk]
        downs = [(1 + i, 0, b) for i, b in enumerate(late)] + ([(11, 0, db // 2)] if opt else [])
    return rooms, ups, downs


@pytest.mark.parametrize("form", ["pack_events", "pack_message", "unpack_message"])
@pytest.mark.parametrize("K", [0, 1, 7, 4097])
@pytest.mark.parametrize("opt", [0, 1])
def test_stage_equals_the_take_sequence(prog, form, K, opt):
    out = run(prog, "stage", form, K, opt)
    tags = [ln[0] for ln in out]
    assert tags == ["up", "down", "full", "carve", "stage", "up", "down", "full"]
    nums = [[int(x) for x in ln[1:]] for ln in out]
    up0, down0, full0, carve, stage, up1, down1, full1 = nums
    rooms, ups, downs = model(form, K, opt)
    offs, o = [], 0
    for b in rooms:
        offs.append(o)
        o += r256(b)
    assert carve == offs + [o], "the literal take sequence against the model"
    assert stage == carve, "Stage gives the offsets and the total of the take sequence"
    assert all(x % 256 == 0 for x in stage)
    pairs = lambda v: list(zip(v[0::2], v[1::2]))
    assert pairs(up0) == pairs(up1) == [(offs[i], b) for i, b in ups if b], "uploads in call order; nothing for an empty or absent array"
    assert pairs(down0) == [(offs[i], b0) for i, b0, _ in downs], "downloads in call order, late ones empty so far"
    assert pairs(down1) == [(offs[i], b1) for i, _, b1 in downs], "... and with the sizes set afterwards"
    assert full0 == full1 == [0]
