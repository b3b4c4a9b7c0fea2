"""Test scaffolding: streams on which find_order's final sort (swirld.py:306, key (consensus timestamp, white ^ signature as a
512-bit integer)) is decided BEHIND the first 8 key bytes — the bytes the device sorts carry (k_order_sort, k_order_sort_big in
csrc/order.hip.h); a round with two events equal in timestamp and in those bytes is left to host_sort_rounds.

A case is a stream (creator, self-parent, other-parent, t, sig) with two changes:

    timestamps   t -> rank(t) // q: runs of q equal values, so that the medians of swirld.py:305 coincide inside a round;
    signatures   the CRAFTED events (all of them, or those of an index window) share bytes 0..7; a share of them (the DEEP
                 ones) also share bytes 8..60 and differ pairwise in bytes 61..63; every other byte stays as drawn.

No two signatures are equal in all 64 bytes (the reference's order among equal keys is its set's iteration order).  The
whitening key of a round is common to its events: equal bytes of `sig` are equal bytes of `white ^ sig`.

`redrawn` gives the same case with bytes 8..63 of the crafted events drawn afresh (not complemented: the complement cancels
against the whitening key of a round with an odd number of famous witnesses): the timestamps, bytes 0..7 and with them every
tie stay, and only what lies behind byte 8 decides differently.  tests/test_order_tie_cases.py proves with the oracle that
every case's order depends on those bytes; tests/test_gpu_order_ties.py runs the HIP path on the same cases.  Never imported
by the product."""
import importlib
import os
from collections import namedtuple

import numpy as np

TIES_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "order_ties")

ALL = None      # the crafted set "all events"; otherwise (a, b, d): the index window [N a / d, N b / d)

# name, source ("golden:<fixture whose stream is taken>" or "synth"), members, events, synth seed / mode / p0 / p1,
# chunk (None: one call), q, crafted set, share of deep events
Case = namedtuple("Case", "name source n N seed mode p0 p1 chunk q window share")

WINDOW = (1, 2, 6)      # [N / 6, N / 3)

CASES = [Case(*row) for row in (
    # ---- recorded from the reference (tests/golden/order_ties, make_order_ties_golden.py): at most 2000 events
    ("ref_n4_chunk7_all", "golden:n4_s6_chunk7", 4, 400, 0, 0, 0, 0, 7, 8, ALL, 2 / 3),
    ("ref_n16_chunk250_all", "golden:n16_s4_chunk250", 16, 2000, 0, 0, 0, 0, 250, 8, ALL, 2 / 3),
    ("ref_n10_stake_all", "golden:n10_s1_stake", 10, 1500, 0, 0, 0, 0, None, 8, ALL, 2 / 3),
    ("ref_n7_chunk13_window", "golden:n7_s2_chunk13", 7, 700, 0, 0, 0, 0, 13, 8, WINDOW, 2 / 3),
    # ---- tie detection: rounds with and without ties in one call (33 members: one mask word; 130: four)
    ("n33_window", "synth", 33, 6000, 301, 0, 0, 0, None, 8, WINDOW, 2 / 3),
    ("n130_window", "synth", 130, 14000, 302, 0, 0, 0, None, 16, WINDOW, 2 / 3),
    # ---- rounds of more than 4096 events (the shape of test_rounds_larger_than_the_lds_sort): k_order_sort_big
    ("n256_big_window", "synth", 256, 70000, 87, 2, 0.35, 0.02, None, 16, (2, 5, 8), 2 / 3),
    # ---- several groups under SW_ORDER_SLAB_MB=1 (test_find_order_table_path_under_its_knobs' smallest shape): the early copy
    ("n100_groups_window", "synth", 100, 60000, 92, 2, 0.3, 0.03, None, 16, WINDOW, 2 / 3),
    # ---- the short output, events that never passed through the host, the forced host sort
    ("n16_all", "synth", 16, 6000, 95, 0, 0, 0, 1500, 8, ALL, 2 / 3),
    # ---- the exact path: forked goldens' streams
    ("forks_n8_all", "golden:n8_s11_forks", 8, 512, 0, 0, 0, 0, None, 8, ALL, 2 / 3),
    ("forks_n12_stake_chunk40_all", "golden:n12_s14_forks_stake_chunk40", 12, 1232, 0, 0, 0, 0, 40, 8, ALL, 2 / 3),
    # ---- medians over duplicate-heavy samples: more than 64 samples per event (four and eight mask words)
    ("n130_q16", "synth", 130, 14000, 311, 0, 0, 0, None, 16, ALL, 2 / 3),
    ("n130_q64", "synth", 130, 14000, 312, 0, 0, 0, None, 64, ALL, 2 / 3),
    ("n300_q16", "synth", 300, 32000, 313, 0, 0, 0, None, 16, ALL, 2 / 3),
    ("n300_q64", "synth", 300, 32000, 314, 0, 0, 0, None, 64, ALL, 2 / 3),
)]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
RECORDED = [c.name for c in CASES if c.name.startswith("ref_")]


def quantise(t, q):
    """rank(t) // q as float64 (ties in t broken by index): finite, non-negative, runs of q equal values"""
    t = np.asarray(t, np.float64)
    rank = np.empty(len(t), np.int64)
    rank[np.argsort(t, kind="stable")] = np.arange(len(t))
    return (rank // int(q)).astype(np.float64)


def crafted_mask(N, window):
    m = np.zeros(N, bool)
    if window is ALL:
        m[:] = True
    else:
        a, b, d = window
        m[N * a // d:N * b // d] = True
    return m


def _unique_rows(sig):
    return len(np.unique(sig, axis=0)) == len(sig)


def craft(stream, q, window=ALL, share=2 / 3, seed=0):
    """(stream with quantised timestamps and crafted signatures, crafted mask, deep mask)"""
    cr, sp, op, t, sig = stream
    N = len(cr)
    rng = np.random.default_rng(77000 + seed)
    sig = np.array(sig, np.uint8).reshape(N, 64).copy()
    crafted = crafted_mask(N, window)
    idx = np.flatnonzero(crafted)
    sig[idx, :8] = rng.integers(0, 256, 8, dtype=np.uint8)
    deep_idx = idx[rng.random(len(idx)) < share]
    sig[deep_idx, 8:61] = rng.integers(0, 256, 53, dtype=np.uint8)
    tail = rng.choice(1 << 24, len(deep_idx), replace=False)      # pairwise distinct in bytes 61..63
    for b, shift in ((61, 16), (62, 8), (63, 0)):
        sig[deep_idx, b] = (tail >> shift) & 0xFF
    deep = np.zeros(N, bool)
    deep[deep_idx] = True
    assert _unique_rows(sig), "two signatures equal in all 64 bytes: the reference's order is not defined"
    return (np.asarray(cr), np.asarray(sp), np.asarray(op), quantise(t, q), sig), crafted, deep


def redrawn(stream, crafted, seed=0):
    """the case with bytes 8..63 of the crafted events drawn afresh"""
    cr, sp, op, t, sig = stream
    rng = np.random.default_rng(88000 + seed)
    sig = sig.copy()
    idx = np.flatnonzero(crafted)
    sig[idx, 8:] = rng.integers(0, 256, (len(idx), 56), dtype=np.uint8)
    assert _unique_rows(sig)
    return cr, sp, op, t, sig


def base_stream(case):
    """(stream before crafting, stake or None)"""
    if case.source.startswith("golden:"):
        from conftest import load_golden
        g = load_golden(case.source[7:])
        assert g["n"] == case.n and len(g["creator"]) == case.N and (g["chunk"] >= case.N) == (case.chunk is None)
        stake = None if (g["stake"] == 1).all() else g["stake"].astype(np.uint64)
        return (g["creator"], g["self_parent"], g["other_parent"], g["t"], g["sig"]), stake
    pkg = importlib.import_module("py-swirld_amd")
    return pkg.synth_hashgraph(case.n, case.N, case.seed, case.mode, case.p0, case.p1), None


def case_seed(case):
    return NAMES.index(case.name)


def build(case):
    """(stream, stake, crafted mask, deep mask) of a case"""
    base, stake = base_stream(case)
    stream, crafted, deep = craft(base, case.q, case.window, case.share, case_seed(case))
    return stream, stake, crafted, deep


def redrawn_of(case, stream, crafted):
    return redrawn(stream, crafted, case_seed(case))


def calls_of(case):
    k = case.chunk or case.N
    return [(a, min(case.N, a + k)) for a in range(0, case.N, k)]


Run = namedtuple("Run", "new_c orders transactions")


def oracle_run(case, stream, stake=None):
    """the oracle through the case's call schedule: new_c and find_order's result per call, and the whole order"""
    from oracle.oracle import Oracle
    o = Oracle(case.n, stake)
    new_c, orders = [], []
    for a, b in calls_of(case):
        o.append_events(*[x[a:b] for x in stream])
        o.divide_rounds(a, b - a)
        nc = [int(r) for r in o.decide_fame()]
        new_c.append(nc)
        orders.append(np.array(o.find_order(nc)))
    return Run(new_c, orders, np.array(o.transactions)), o


def k8_of(sig):
    """bytes 0..7 of every signature as one big-endian integer: the key the device sorts carry, up to the round's whitening"""
    return np.ascontiguousarray(np.asarray(sig, np.uint8)[:, :8]).view(">u8").reshape(-1).astype(np.uint64)


def tied_rounds(events, round_received, consensus_time, sig):
    """The received rounds, among those of `events`, that hold two events equal in consensus time and in bytes 0..7 of the
    signature (the rounds host_sort_rounds has to sort), as a sorted array; `round_received` / `consensus_time` are indexed
    by event."""
    ev = np.asarray(events, np.int64)
    if len(ev) == 0:
        return np.zeros(0, np.int64)
    rr = np.asarray(round_received)[ev].astype(np.int64)
    ct = np.asarray(consensus_time, np.float64)[ev]
    assert (rr >= 0).all() and np.isfinite(ct).all() and (ct >= 0).all()      # (no -0.0: equal values have equal bits)
    k8 = k8_of(np.asarray(sig)[ev])
    o = np.lexsort((k8, ct, rr))
    rr, ct, k8 = rr[o], ct[o], k8[o]
    same = (rr[1:] == rr[:-1]) & (ct[1:] == ct[:-1]) & (k8[1:] == k8[:-1])
    return np.unique(rr[1:][same])


def load_recorded(name):
    with np.load(os.path.join(TIES_DIR, name + ".npz")) as z:
        return {k: z[k] for k in z.files}
