#!/usr/bin/env python3
"""Records what the UNMODIFIED reference computes for every case of tests/test_oracle_vs_reference_random.py
into tests/golden/random/{plain,forked}_<seed>.npz: the input stream, the call schedule, decide_fame's and
find_order's result per call (or the call at which find_order raised IndexError, swirld.py:305) and the final
Node state.  Needs the reference tree (tests/refharness.py); the fixtures are committed.

Usage:  python tests/golden/make_random_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from refharness import RefRun  # noqa: E402
from synth_util import synth  # noqa: E402
from test_oracle_vs_reference_random import RANDOM_DIR, forked_case, plain_case  # noqa: E402


def record(n, stream, stake, chunk):
    cr, sp, op, t, sig = stream
    N = len(cr)
    ref = RefRun(n, stake)
    nc_flat, nc_off, tx_flat, tx_off = [], [0], [], [0]
    index_error_call = -1
    for i, a in enumerate(range(0, N, chunk)):
        b = min(N, a + chunk)
        ref.append(cr[a:b], sp[a:b], op[a:b], t[a:b], sig[a:b])
        ref.divide_rounds(a, b - a)
        nc = list(ref.decide_fame())
        nc_flat += nc
        nc_off.append(len(nc_flat))
        try:
            tx_flat += list(ref.find_order(nc))
        except IndexError:
            index_error_call = i
            tx_off.append(len(tx_flat))
            break
        tx_off.append(len(tx_flat))
    out = dict(n=np.int32(n), stake=np.zeros(0, np.int64) if stake is None else np.asarray(stake, np.int64),
               chunk=np.int64(chunk), creator=np.asarray(cr), self_parent=np.asarray(sp), other_parent=np.asarray(op),
               t=np.asarray(t), sig=np.asarray(sig), index_error_call=np.int32(index_error_call),
               new_c_flat=np.array(nc_flat, np.int32), new_c_off=np.array(nc_off, np.int32),
               tx_flat=np.array(tx_flat, np.int32), tx_off=np.array(tx_off, np.int64))
    if index_error_call < 0:
        ex = ref.extract()
        wo_flat = np.concatenate(ex["wit_order"]) if ex["wit_order"] else np.zeros(0, np.int32)
        out.update(round=ex["round"], can_see=ex["can_see"], witnesses=ex["witnesses"],
                   wit_order_flat=wo_flat.astype(np.int32),
                   wit_order_off=np.cumsum([0] + [len(o) for o in ex["wit_order"]]).astype(np.int32),
                   famous=ex["famous"], consensus=ex["consensus"], transactions=ex["transactions"], tbd=ex["tbd"],
                   n_votes=np.int64(len(ex["votes"])))
    else:
        out.update(wit_order_flat=np.zeros(0, np.int32), wit_order_off=np.zeros(1, np.int32))
    return out


def main():
    os.makedirs(RANDOM_DIR, exist_ok=True)
    for kind, make, seeds in (("plain", plain_case, range(24)), ("forked", forked_case, range(16))):
        for seed in seeds:
            n, stream, stake, chunk, lanes = make(synth, seed)
            out = record(n, stream, stake, chunk)
            if lanes is not None:
                out["lanes"] = np.bool_(lanes)
            path = os.path.join(RANDOM_DIR, "%s_%02d.npz" % (kind, seed))
            np.savez_compressed(path, **out)
            print("%-10s n=%2d N=%4d chunk=%4d calls=%3d index_error_call=%3d  %6.1f KB" % (
                "%s_%02d" % (kind, seed), n, len(stream[0]), chunk, len(out["new_c_off"]) - 1, int(out["index_error_call"]),
                os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
