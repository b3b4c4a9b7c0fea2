#!/usr/bin/env python3
"""Records what the UNMODIFIED reference Node computes for tests/test_node_vs_reference.py into
tests/golden/node/*.json.gz: the end state of every node of its own simulation (run in a child process
under the test's fixed hash seed), its accept / reject decisions on valid and malformed events, and an
observer's results per call and end state on forked hashgraphs.  Needs the reference tree
(tests/refharness.py); the fixtures are committed.

Usage:  python tests/golden/make_node_golden.py
"""
import contextlib
import gzip
import io
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import refharness  # noqa: E402
import test_node_vs_reference as T  # noqa: E402


def save(name, obj):
    os.makedirs(T.NODE_DIR, exist_ok=True)
    path = os.path.join(T.NODE_DIR, name + ".json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(obj, separators=(",", ":")).encode())
    print("%-28s %6.1f KB" % (name, os.path.getsize(path) / 1024))


def reference_simulation(n, turns, seed):
    sw = refharness.import_reference()
    import pysodium  # the stand-in of tests/_pysodium_standin
    pysodium.set_rng(T._rng_bytes(seed))
    sw.time, sw.dumps = T._clock(), T._class_free_dumps
    with contextlib.redirect_stdout(io.StringIO()):
        nodes = sw.test(n, turns)
    return T.simulation_summary(nodes)


def reference_is_valid_event():
    sw = refharness.import_reference()
    import pysodium
    sw.dumps, sw.time = T._class_free_dumps, T._clock()
    kps = [pysodium.crypto_sign_seed_keypair(bytes([i]) * 32) for i in range(3)]
    stake = {kp[0]: 1 for kp in kps}
    ref = [sw.Node(kp, {}, 3, stake) for kp in kps]
    for a in ref[1:]:
        ref[0].add_event(a.head, a.hg[a.head])
    r0 = ref[0]
    good_h, good = r0.new_event(b"x", (r0.head, ref[1].head))
    cases = [("well-formed", good_h, good), ("wrong hash", b"\0" * 32, good), ("tampered payload", good_h, good._replace(d=b"z")),
             ("tampered timestamp", good_h, good._replace(t=good.t + 1)), ("bad signature", good_h, good._replace(s=bytes(64)))]

    def signed(p):
        ev = sw.Event(b"x", p, good.t, r0.pk, b"")
        ev = ev._replace(s=pysodium.crypto_sign_detached(T._class_free_dumps(tuple(ev[:-1])), r0.sk))
        return sw.crypto_generichash(T._class_free_dumps(ev)), ev
    cases.append(("parents swapped (first is not the self-parent)",) + signed((ref[1].head, r0.head)))
    cases.append(("other-parent is mine",) + signed((r0.head, r0.head)))
    cases.append(("unknown parent",) + signed((r0.head, b"\x07" * 32)))
    cases.append(("one parent",) + signed((r0.head,)))
    return sorted([name, bool(r0.is_valid_event(h, ev))] for name, h, ev in cases)


def reference_forked(n, steps, seed, n_forks):
    sw = refharness.import_reference()
    import pysodium
    sw.dumps, sw.time = T._class_free_dumps, T._clock()
    obs, calls = T.forked_run(pysodium.crypto_sign_seed_keypair, n, steps, seed, n_forks,
                              lambda kp, n_, stake: sw.Node(kp, {}, n_, stake))
    return {"calls": calls, "state": T.observer_state(obs)}


def main():
    for n, turns, seed in T.SIM_CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--sim", str(n), str(turns), str(seed)], check=True,
                           capture_output=True, text=True, env=dict(os.environ, PYTHONHASHSEED=T.HASH_SEED))
        save("sim_%d_%d_%d" % (n, turns, seed), json.loads(p.stdout.strip().splitlines()[-1]))
    save("is_valid_event", reference_is_valid_event())
    for case in T.FORK_CASES:
        save("forked_%d_%d_%d_%d" % case, reference_forked(*case))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--sim"]:
        print(json.dumps(reference_simulation(*[int(a) for a in sys.argv[2:5]])))
    else:
        main()
