#!/usr/bin/env python3
"""Records what the UNMODIFIED reference computes for the recorded cases of tests/order_tie_cases.py (quantised timestamps,
signatures that share their first 8 bytes and mostly their first 61: find_order's final sort, swirld.py:306, is decided by
the last bytes of the 512-bit key) into tests/golden/order_ties/<case>.npz: the input stream, the stake, the call schedule,
and per call decide_fame's result and what find_order appended to the order.  Needs the reference tree
(tests/refharness.py); the fixtures are committed.

Usage:  python tests/golden/make_order_ties_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import order_tie_cases as T  # noqa: E402
from refharness import RefRun  # noqa: E402


def record(case):
    stream, stake, crafted, deep = T.build(case)
    cr, sp, op, t, sig = stream
    ref = RefRun(case.n, stake)
    calls = T.calls_of(case)
    nc_flat, nc_off, tx_flat, tx_off = [], [0], [], [0]
    for a, b in calls:
        ref.append(cr[a:b], sp[a:b], op[a:b], t[a:b], sig[a:b])
        ref.divide_rounds(a, b - a)
        nc = list(ref.decide_fame())
        nc_flat += nc
        nc_off.append(len(nc_flat))
        tx_flat += list(ref.find_order(nc))
        tx_off.append(len(tx_flat))
    return dict(n=np.int32(case.n), stake=np.ones(case.n, np.int64) if stake is None else np.asarray(stake, np.int64),
                sched=np.array([b - a for a, b in calls], np.int64), q=np.int32(case.q), crafted=crafted, deep=deep,
                creator=np.asarray(cr, np.int32), self_parent=np.asarray(sp, np.int32), other_parent=np.asarray(op, np.int32),
                t=np.asarray(t, np.float64), sig=np.asarray(sig, np.uint8),
                new_c_flat=np.array(nc_flat, np.int32), new_c_off=np.array(nc_off, np.int32),
                tx_flat=np.array(tx_flat, np.int32), tx_off=np.array(tx_off, np.int64))


def main():
    os.makedirs(T.TIES_DIR, exist_ok=True)
    for name in T.RECORDED:
        case = T.BY_NAME[name]
        assert case.N <= 2000
        out = record(case)
        path = os.path.join(T.TIES_DIR, name + ".npz")
        np.savez_compressed(path, **out)
        print("%-24s n=%2d N=%4d calls=%3d ordered=%4d  %6.1f KB" % (name, case.n, case.N, len(out["sched"]), len(out["tx_flat"]),
                                                                     os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
