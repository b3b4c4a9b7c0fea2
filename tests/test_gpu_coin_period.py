"""GPU (-m gpu): coin rounds (swirld.py:267-272) at coin periods other than the reference's own 6, on every path that reads
`coin_period`.  At period 2 or 3 the coin branch is the second or third level of EVERY election, so hashgraphs of a few
hundred events hold thousands of coin votes and three or four rounds are enough for the wide kernels; at period 6 the same
branch is reached only by elections that stay open for six rounds.

 a. the fixtures of tests/golden/coin_period/ — the UNMODIFIED reference run with its C set to 1, 2, 3 or 50 — through
    Hashgraph(coin_period=k) on their recorded schedules: every table, round received and consensus time bit for bit, and
    every entry of the reference's `votes` through sw_get_vote and through the bulk export;
 b. every election kernel instance (k_elections<1..16>, k_elections_tiled<2..16> at its workgroup sizes), unit and
    weighted stake, periods 2 and 3, against the oracle (pinned to those fixtures by tests/test_coin_period_host.py);
 c. the coin bits of events that never passed through the host append: device-memory append, payload ingest, signed-event
    creation, tiny appends, the windowed table, and a pass after rewind;
 d. the exact path with its history on the forked fixtures;
 e. batches; f. the partitioned decide_fame and sw_split_link; g. the degenerate periods; h. Node and DeviceNetwork.

Whether a case holds coin votes at all is always asserted from the reference's or the oracle's counters, never from the
device's.  No torch here (see tests/test_gpu_ingest_device.py)."""
import importlib
import random

import numpy as np
import pytest

import batch_cases
import coin_period_cases as cp
import model_payload as mp
import oracle_pool as op_
from oracle.oracle import Oracle
from test_batch_host import same_bits
from test_gpu_batch import assert_same as batch_assert_same
from test_gpu_exact_history import check_consensus, check_lookups, entries_dict
from test_gpu_parity import assert_state_equal
from test_gpu_payload import Hip, dev_ingest
from test_gpu_votes import check_table, entries, lookup, sample_pairs

pytestmark = pytest.mark.gpu

NAMES = cp.names()
FORKFREE = [nm for nm in NAMES if not cp.is_forked(nm)]
FORKED = [nm for nm in NAMES if cp.is_forked(nm)]
FAME_COUNTERS = ("voter_evals", "majority_evals", "coin_votes", "coin_flips")


@pytest.fixture
def hip(pkg):
    h = Hip(pkg)
    yield h
    h.free()


def as_set(tr):
    return set(map(tuple, np.asarray(tr).tolist()))


def slices(g, a, b):
    return tuple(g[k][a:b] for k in ("creator", "self_parent", "other_parent", "t", "sig"))


def run_fixture(h, g, t=None):
    """The fixture's recorded schedule: decide_fame's return and the transactions of every call."""
    for call, (a, b) in enumerate(g["batches"]):
        cr, sp, op, tt, sig = slices(g, a, b)
        h.append_events(cr, sp, op, tt if t is None else t[a:b], sig)
        h.divide_rounds(a, b - a)
        nc = h.decide_fame()
        assert list(nc) == cp.new_c_of(g, call), "new_c of call %d" % call
        tx = h.find_order(nc)
        if t is None:
            assert list(tx) == cp.tx_of(g, call), "find_order of call %d" % call


def oracle_of(g, period=None):
    o = Oracle(g["n"], g["stake"], g["coin_period"] if period is None else period)
    for a, b in g["batches"]:
        o.append_events(*slices(g, a, b))
        o.divide_rounds(a, b - a)
        o.find_order(o.decide_fame())
    return o


def oracle_votes(o):
    """Every entry of the oracle's votes dict as (y, x, v) — it is asked pair by pair, every (witness, earlier witness)."""
    wit, rnd = o.witnesses(), o.round
    slots = [int(e) for e in wit[wit >= 0]]
    out = set()
    for y in slots:
        for x in slots:
            if rnd[x] < rnd[y]:
                v = o.vote(y, x)
                if v >= 0:
                    out.add((y, x, v))
    assert len(out) == o.num_votes, "every entry of the oracle is a (witness, earlier witness) pair"
    return out


def check_votes_both_ways(h, votes, wit, rnd, cr, seed=0, absent=1500):
    """`votes` ([K, 3] or a set of (y, x, v): the complete dict) against sw_get_vote — every entry, and pairs without one —
    and against the bulk export as a set."""
    triples = np.array(sorted(map(tuple, np.asarray(list(votes) if isinstance(votes, set) else votes).tolist())), np.int64).reshape(-1, 3)
    have = {(int(y), int(x)) for y, x, _ in triples}
    assert len(have) == len(triples)
    for y, x, v in triples:
        assert h.vote(rnd[y], cr[y], rnd[x], cr[x]) == v, "votes[%d][%d]" % (y, x)
    R, n = wit.shape
    rng = np.random.default_rng(seed)
    checked = 0
    for _ in range(4 * absent if R > 1 else 0):
        rv = int(rng.integers(1, R)); rc = int(rng.integers(0, rv))
        mv = int(rng.integers(0, n)); mc = int(rng.integers(0, n))
        y, x = wit[rv, mv], wit[rc, mc]
        if y < 0 or x < 0 or (int(y), int(x)) in have:
            continue
        assert h.vote(rv, mv, rc, mc) == -1, "votes[%d][%d] has no entry" % (y, x)
        checked += 1
        if checked >= absent:
            break
    table = h.export_votes()
    check_table(h, table)
    tr = h.votes_triples()
    assert len(tr) == len(triples) == entries(table)
    assert as_set(tr) == as_set(triples)
    return checked


# ---- a. the reference's fixtures, fork-free ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORKFREE)
def test_reference_fixture(pkg, name):
    g = cp.load(name)
    N = len(g["creator"])
    h = pkg.Hashgraph(g["n"], g["stake"], coin_period=g["coin_period"])
    run_fixture(h, g)
    assert not h.exact
    assert np.array_equal(h.heights(), g["height"])
    assert_state_equal(h, g["round"], g["can_see"], g["witnesses"], g["famous"], g["consensus"])
    for r, order in enumerate(g["wit_order"]):
        assert np.array_equal(h.witness_order(r), order), "dict order of witnesses[%d]" % r
    assert np.array_equal(h.famous_events(), g["famous"])
    assert np.array_equal(h.transactions(), g["transactions"])
    assert np.array_equal(h.round_received(), g["asis_round_received"])
    assert same_bits(h.consensus_time(), g["asis_consensus_time"])
    c = h.counters()
    if len(g["batches"]) == 1:
        co = oracle_of(g).counters()
        assert {k: c[k] for k in FAME_COUNTERS} == {k: co[k] for k in FAME_COUNTERS}
        assert (c["coin_votes"], c["coin_flips"]) == (g["coin_votes"], g["coin_flips"]), "the reference's own counts"
    absent = check_votes_both_ways(h, g["votes"], g["witnesses"], g["round"], g["creator"])
    # (where nothing is ever decided, every witness holds an entry on every earlier witness)
    assert absent > 100 or (g["famous"] == -1).all()
    if name in cp.NO_ELECTION:
        assert len(g["votes"]) == 0 and N == 600
    h.close()


# ---- b. every election kernel instance against the oracle ------------------------------------------------------------------------
# The shapes are tests/oracle_pool.py's COIN_SHAPES.  Measured with the oracle alone (coin votes / of those by the signature
# bit; rounds decided; largest voter distance), unit stake | stake 3 on every 7th member:
#                 period 2                                     period 3
#   n40    14 080 /  6 829, 1, 6 |  8 520 /  1 525, 1, 6    1 320 /   640, 4, 5 |   480 /    54, 3, 4
#   n64    26 512 /  7 629, 3, 5 | 20 016 /  1 659, 2, 5    2 096 /   512, 4, 5 |   480 /    22, 3, 4
#   n65    36 170 / 12 799, 2, 8 | 26 382 /  2 741, 2, 6    2 855 /   808, 4, 7 |   906 /   104, 4, 5
#   n130  139 204 / 75 668, 0, 7 | 44 368 /  9 078, 0, 4   19 156 / 6 826, 2, 7 | 2 681 /   398, 1, 4
#   n256  344 266 /123 693, 1, 7 |179 421 / 33 235, 0, 4   27 589 / 6 632, 3, 7 | 5 061 / 1 019, 1, 4
#   n300  180 000 / 38 609, 0, 3 |180 000 / 11 704, 0, 3   10 500 / 1 291, 0, 3 | 4 500 /   328, 0, 3
#   n520  424 840 / 94 414, 0, 3 |      (28 000 events)    16 632 / 2 681, 0, 3 | 8 208 /   248, 0, 3
# At 300 and 520 members a round decided AFTER a coin round was not reachable with an oracle run of seconds (a round is
# some 5 000 and 8 000 events there): the coin-vote condition alone is asserted for them.
# kernel instance by (shape, SW_ELECT_IMPL, SW_ELECT_CG), from fame_launch (csrc/swirld_hip.hip):
KERNELS = [
    ("n40", None, None),     # k_elections<1>
    ("n64", None, None),     # k_elections<1>, all 64 lanes candidates
    ("n65", None, None),     # k_elections_tiled<2, ., 128>
    ("n130", None, None),    # k_elections_tiled<4, ., 128>
    ("n130", None, "64"),    # k_elections_tiled<4, ., 64>
    ("n130", None, "256"),   # k_elections_tiled<4, ., 256>
    ("n256", None, None),    # k_elections_tiled<4, ., 128>, every member a candidate
    ("n256", None, "64"),
    ("n256", None, "256"),
    ("n300", None, None),    # k_elections_tiled<8, ., 128>: voter masks read from global memory
    ("n520", None, None),    # k_elections_tiled<16, ., 64>
    ("n65", "0", None),      # k_elections<2>
    ("n130", "0", None),     # k_elections<4>
    ("n300", "0", None),     # k_elections<8>
    ("n520", "0", None),     # k_elections<16>
]
DECIDES_AFTER_A_COIN_ROUND = ("n65", "n130", "n256")   # at period 3 (unit and weighted)


def pool_name(shape, period, weighted):
    return "%s%s/c%d/%s" % (op_.COIN_PERIOD, shape, period, "weighted" if weighted else "unit")


@pytest.fixture(scope="module", autouse=True)
def oracle_runs(oracle_pool):
    """Every oracle run of section b, started in the pool's threads when the first test of the file begins: the 520-member
    ones take some 15 s each and overlap sections a and b's smaller cases."""
    for shape in sorted(op_.COIN_SHAPES, key=lambda s: -op_.COIN_SHAPES[s][0]):
        for period in (2, 3):
            for weighted in (False, True):
                oracle_pool.start(pool_name(shape, period, weighted))
    return oracle_pool


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("period", [2, 3])
@pytest.mark.parametrize("shape,impl,cg", KERNELS, ids=["%s%s%s" % (s, "-impl" + i if i else "", "-cg" + c if c else "") for s, i, c in KERNELS])
def test_election_kernels(pkg, oracle_runs, monkeypatch, shape, impl, cg, period, weighted):
    run = oracle_runs.get(pool_name(shape, period, weighted))
    o, n, N = run.oracle, run.n, run.N
    co = o.counters()
    # ---- the case holds what it is here for: from the oracle alone
    assert co["coin_votes"] > 0 and 0 < co["coin_flips"] < co["coin_votes"], co
    if period == 3 and shape in DECIDES_AFTER_A_COIN_ROUND:
        assert run.new_c and co["max_vote_distance"] > 3, "a round decided after a coin round"
    if weighted:
        unit = oracle_runs.get(pool_name(shape, period, False))
        k = min(N, unit.N)
        assert not (run.stake == 1).all() and not np.array_equal(o.round[:k], unit.oracle.round[:k]), "the stakes change the pass"
    # ---- the device
    if impl is not None:
        monkeypatch.setenv("SW_ELECT_IMPL", impl)
    if cg is not None:
        monkeypatch.setenv("SW_ELECT_CG", cg)
    h = pkg.Hashgraph(n, run.stake, coin_period=period)
    h.append_events(*run.stream)
    h.divide_rounds(0, N)
    nc = [int(r) for r in h.decide_fame()]
    assert nc == run.new_c
    assert np.array_equal(h.find_order(nc), run.order)
    assert_state_equal(h, o.round, o.can_see, o.witnesses(), o.famous_by_event, o.consensus())
    c = h.counters()
    assert {k: c[k] for k in FAME_COUNTERS} == {k: co[k] for k in FAME_COUNTERS}
    assert c["rounds"] == co["rounds"]
    # ---- the votes: the bulk export against the oracle, and against sw_get_vote on a sample
    table = h.export_votes()
    check_table(h, table)
    tr = h.votes_triples()
    assert len(tr) == o.num_votes == entries(table)
    at = lookup(h, table)
    cr, rnd, wit = run.stream[0], o.round, o.witnesses()
    pairs = sample_pairs(wit, tr, np.random.default_rng(period), 1500, 1500)
    present = coin_level = 0
    for y, x in pairs:
        got = at(y, x, cr)
        assert got == o.vote(y, x), "votes[%d][%d]" % (y, x)
        present += got >= 0
        coin_level += got >= 0 and (rnd[y] - rnd[x]) % period == 0
    assert present >= min(1500, len(tr)) and coin_level > 0, "entries of coin rounds were among those compared"
    for y, x in pairs[:150] + pairs[-150:]:
        assert at(y, x, cr) == h.vote(int(rnd[y]), int(cr[y]), int(rnd[x]), int(cr[x]))
    h.close()


# ---- c. coin bits of events that never passed through the host append -----------------------------------------------------------
SMALL = "n7_s2_chunk13_c3"     # 7 members, 700 events, period 3: 7 661 coin votes in the reference's own run


def growing_cuts(N, first=50):
    """Calls that each hold more than an eighth of the events stored so far: what the device-memory append takes on the
    device (a smaller one goes to the host path, csrc/swirld_hip.hip: append_device_body)."""
    cuts = [0, first]
    while cuts[-1] < N:
        nxt = cuts[-1] + cuts[-1] // 8 + 1
        if N - nxt < nxt // 8 + 1:      # (a remainder too small for a call of its own joins this one)
            nxt = N
        cuts.append(min(N, nxt))
    return list(zip(cuts[:-1], cuts[1:]))


def compare_call(h, o, nc, what):
    nco = o.decide_fame()
    assert list(nc) == list(nco), what + ": new_c"
    assert list(h.find_order(nc)) == list(o.find_order(nco)), what + ": find_order"
    assert np.array_equal(h.rounds(), o.round), what + ": rounds"
    wit = h.witnesses()
    assert np.array_equal(wit, o.witnesses()), what + ": witnesses"
    assert np.array_equal(h.famous(), o.famous_table()), what + ": famous"
    assert np.array_equal(h.consensus(), o.consensus()), what + ": consensus"


def compare_end(h, o, cr, first_row=0):
    N = o.N
    assert np.array_equal(h.can_see(first_row, N - first_row), o.can_see[first_row:])
    assert np.array_equal(h.transactions(), o.transactions)
    co = o.counters()
    assert co["coin_votes"] > 0 and 0 < co["coin_flips"] < co["coin_votes"], co
    check_votes_both_ways(h, oracle_votes(o), o.witnesses(), o.round, cr, absent=300)


def dev_append(h, hip, cr, sp, op, t, sig):
    try:
        h.append_events_device(hip.up(cr, np.int32), hip.up(sp, np.int32), hip.up(op, np.int32), hip.up(t, np.float64),
                               hip.up(sig, np.uint8), count=len(cr))
    finally:
        hip.free()


def test_device_memory_append_then_rewind(pkg, hip):
    g = cp.load(SMALL)
    n, N, k = g["n"], len(g["creator"]), g["coin_period"]
    h, o = pkg.Hashgraph(n, coin_period=k), Oracle(n, None, k)
    calls = growing_cuts(N)
    for a, b in calls:
        dev_append(h, hip, *slices(g, a, b))
        o.append_events(*slices(g, a, b))
        for d in (h, o):
            d.divide_rounds(a, b - a)
        compare_call(h, o, h.decide_fame(), "call [%d, %d)" % (a, b))
    st = h.ingest_stats()
    assert st["device_batches"] == len(calls) and st["fallback_batches"] == 0, st   # (a run that fell back would prove nothing here)
    compare_end(h, o, g["creator"])
    # ---- after rewind(): the events and their coin bits stay, the voting state is built again, in one call
    before = h.counters()
    h.rewind()
    h.divide_rounds(0, N)
    nc = h.decide_fame()
    one = Oracle(n, None, k)
    one.append_events(*slices(g, 0, N))
    one.divide_rounds(0, N)
    compare_call(h, one, nc, "one call after rewind")
    compare_end(h, one, g["creator"])
    c, co = h.counters(), one.counters()
    assert {x: c[x] - before[x] for x in FAME_COUNTERS} == {x: co[x] for x in FAME_COUNTERS}, "the counters run on over a rewind"
    h.close()


def test_payload_ingest_with_shuffled_payloads(pkg, hip):
    g = cp.load(SMALL)
    n, N, k = g["n"], len(g["creator"]), g["coin_period"]
    cr, sp, op, t, sig = slices(g, 0, N)
    h, o = pkg.Hashgraph(n, coin_period=k), Oracle(n, None, k)
    rng = np.random.default_rng(5)
    dense_of = np.full(N, -1, np.int64)      # stream event -> dense index in the context (a payload is numbered by acceptance wave)
    moved = 0
    for a, b in growing_cuts(N):
        idx = rng.permutation(np.arange(a, b))
        out, stored = dev_ingest(h, hip, mp.from_stream(cr, sp, op, idx.tolist()), t[idx], sig[idx])
        assert stored == b - a and sorted(out.tolist()) == list(range(a, b))
        dense_of[idx] = out
        moved += int((out != idx).sum())
        inv = np.empty(b - a, np.int64)      # dense index - a -> stream event
        inv[out - a] = idx
        relabel = lambda p: np.where(p >= 0, dense_of[np.maximum(p, 0)], -1).astype(np.int32)   # noqa: E731
        o.append_events(cr[inv], relabel(sp[inv]), relabel(op[inv]), t[inv], sig[inv])
        for d in (h, o):
            d.divide_rounds(a, b - a)
        compare_call(h, o, h.decide_fame(), "call [%d, %d)" % (a, b))
    assert moved > 0, "the payloads were shuffled: the dense order is not the stream's"
    inv_all = np.argsort(dense_of)
    compare_end(h, o, cr[inv_all])
    h.close()


def test_created_events_carry_the_coin_bits_of_their_own_signatures(pkg):
    g = cp.load(SMALL)
    n, N, k = g["n"], len(g["creator"]), g["coin_period"]
    cr, sp, op, t, _ = slices(g, 0, N)
    seeds = [bytes([91, m]) + bytes(30) for m in range(n)]
    h, o = pkg.Hashgraph(n, coin_period=k), Oracle(n, None, k)
    h.set_member_keys([pkg.node.crypto.sign_seed_keypair(s)[0] for s in seeds])
    h.set_signing_seeds(list(range(n)), seeds)
    sigs = np.zeros((N, 64), np.uint8)
    for a, b in [(0, 1), (1, 40)] + [(x, min(N, x + 33)) for x in range(40, N, 33)]:
        first, _, sig = h.create_events(cr[a:b], sp[a:b], op[a:b], t[a:b], [None] * (b - a), want_ids=True)
        assert first == a
        sigs[a:b] = sig
        o.append_events(cr[a:b], sp[a:b], op[a:b], t[a:b], sig)
        for d in (h, o):
            d.divide_rounds(a, b - a)
        compare_call(h, o, h.decide_fame(), "call [%d, %d)" % (a, b))
    # the signatures as the context STORES them (what its coin bits were taken from), read back through the sync export
    x = h.export_payload(N - 1)
    assert len(x["event"]) > N // 2 and np.array_equal(x["sig"], sigs[x["event"]])
    bits = sigs[:, 0] >> 7
    assert 0.3 < bits.mean() < 0.7 and not np.array_equal(sigs, g["sig"]), "Ed25519's own bits, not the stream's"
    compare_end(h, o, cr)
    h.close()


@pytest.mark.parametrize("window", [False, True], ids=["plain", "windowed"])
def test_tiny_appends(pkg, window):
    """One event per call — the small-append kernel writes the coin bit — and the same with the windowed can_see table."""
    g = cp.load(SMALL)
    n, N, k = g["n"], len(g["creator"]), g["coin_period"]
    h, o = pkg.Hashgraph(n, coin_period=k), Oracle(n, None, k)
    if window:
        h.set_window(True)
    for a in range(N):
        for d in (h, o):
            d.append_events(*slices(g, a, a + 1))
            d.divide_rounds(a, 1)
        nc, nco = h.decide_fame(), o.decide_fame()
        assert list(nc) == list(nco), a
        assert list(h.find_order(nc)) == list(o.find_order(nco)), a
    assert np.array_equal(h.rounds(), o.round)
    assert np.array_equal(h.famous(), o.famous_table())
    assert np.array_equal(h.consensus(), o.consensus())
    assert o.consensus().sum() >= 3, "rounds were decided, after coin rounds"
    compare_end(h, o, g["creator"], first_row=h.window()[0] if window else 0)
    h.close()


# ---- d. the exact path and its history ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["asis", "wallclock"])
@pytest.mark.parametrize("name", FORKED)
def test_forked_fixture_on_the_exact_path_with_history(pkg, hip, name, variant):
    g = cp.load(name)
    N = len(g["creator"])
    t = g["t"] if variant == "asis" else g["wallclock_t"]
    tx_fix = g["transactions"] if variant == "asis" else g["wallclock_transactions"]
    h = pkg.Hashgraph(g["n"], g["stake"], coin_period=g["coin_period"])
    h.set_exact_history()
    run_fixture(h, g, None if variant == "asis" else t)
    assert h.exact and h.votes_available
    assert np.array_equal(h.heights(), g["height"])
    assert np.array_equal(h.rounds(), g["round"])
    assert np.array_equal(h.can_see(), g["can_see"])
    wit = h.witnesses()
    assert np.array_equal(wit, g["witnesses"])
    for r, order in enumerate(g["wit_order"]):
        assert np.array_equal(h.witness_order(r), order), "dict order of witnesses[%d]" % r
    fam, m = h.famous(), wit >= 0
    assert np.array_equal(fam[m], g["famous"][wit[m]]) and (fam[~m] == -1).all()
    assert np.array_equal(h.consensus(), g["consensus"])
    check_consensus(h, hip, N, tx_fix, g[variant + "_round_received"], g[variant + "_consensus_time"], g["creator"])
    ref = {(int(y), int(x)): int(v) for y, x, v in g["votes"]}
    assert g["coin_votes"] > 0 and 0 < g["coin_flips"] < g["coin_votes"]
    got = entries_dict(h)
    assert got.keys() == ref.keys()
    assert got == ref
    check_lookups(h, ref, N, 3)
    h.close()


@pytest.mark.parametrize("name", FORKED)
def test_forked_fixture_on_the_exact_path_without_history(pkg, name):
    g = cp.load(name)
    h = pkg.Hashgraph(g["n"], g["stake"], coin_period=g["coin_period"])
    run_fixture(h, g)
    assert h.exact
    assert np.array_equal(h.rounds(), g["round"])
    wit = h.witnesses()
    assert np.array_equal(wit, g["witnesses"])
    assert np.array_equal(h.famous()[wit >= 0], g["famous"][wit[wit >= 0]])
    assert np.array_equal(h.consensus(), g["consensus"])
    assert np.array_equal(h.transactions(), g["transactions"])
    c = h.counters()
    if len(g["batches"]) == 1:
        assert (c["coin_votes"], c["coin_flips"]) == (g["coin_votes"], g["coin_flips"])
    h.close()


# ---- e. batches --------------------------------------------------------------------------------------------------------------------
BATCH_N = 4
BATCH_FIXTURES = {1: ["n4_s1_batch_c1"], 2: ["n4_s1_batch_c2", "n4_s5_chunk1_c2"], 3: ["n4_s1_batch_c3"]}
BATCH_RANDOM = [(350, 61, 5, (1, 350)), (350, 62, 0, (1, 40)), (300, 63, 9, (20, 120)), (260, 64, 4, (1, 9))]   # events, seed, forks, call sizes


@pytest.mark.parametrize("period", [1, 2, 3])
def test_batch(pkg, period):
    """The 4-member fixtures of this period on their recorded schedules beside random forked hashgraphs under ragged ones,
    in ONE batch created with the period; every step read through step_arrays()."""
    n = BATCH_N
    fx = [cp.load(nm) for nm in BATCH_FIXTURES[period]]
    assert all(g["n"] == n and g["coin_period"] == period for g in fx)
    streams = [slices(g, 0, len(g["creator"])) for g in fx]
    scheds = [[b - a for a, b in g["batches"]] for g in fx]
    expect = [[(cp.new_c_of(g, i), cp.tx_of(g, i)) for i in range(len(g["batches"]))] for g in fx]
    records = []
    for N, seed, forks, sizes in BATCH_RANDOM:
        s = batch_cases.forked_stream(n, N, seed, forks)
        sched = batch_cases.ragged_schedule(len(s[0]), seed, *sizes)
        rec = batch_cases.Record(n, s, sched, coin_period=period)
        assert rec.failed_call is None
        co = rec.o.counters()
        assert co["coin_votes"] > 0 and 0 < co["coin_flips"] < co["coin_votes"], co
        streams.append(s); scheds.append(sched); expect.append(rec.calls); records.append(rec)
    B = len(streams)
    hb = pkg.HashgraphBatch(B, n, coin_period=period, cap_events=max(len(s[0]) for s in streams))
    pos, call = [0] * B, [0] * B
    rr_log = [[] for _ in range(B)]
    ts_log = [[] for _ in range(B)]
    while any(call[b] < len(scheds[b]) for b in range(B)):
        parts, K = [None] * B, np.zeros(B, np.int64)
        for b in range(B):
            if call[b] < len(scheds[b]):
                K[b] = scheds[b][call[b]]
                parts[b] = tuple(x[pos[b]:pos[b] + K[b]] for x in streams[b])
        hb.append(parts)
        out = hb.step_arrays(K)
        assert out.n_failed == 0
        for b in range(B):
            r = out.rounds[out.rounds_off[b]:out.rounds_off[b + 1]]
            ev = out.event[out.tx_off[b]:out.tx_off[b + 1]]
            if not K[b]:
                assert not out.took[b] and len(r) == 0 and len(ev) == 0
                continue
            assert out.took[b]
            assert (list(r), list(ev)) == (list(expect[b][call[b]][0]), list(expect[b][call[b]][1])), "hashgraph %d, call %d" % (b, call[b])
            rr_log[b] += out.round_received[out.tx_off[b]:out.tx_off[b + 1]].tolist()
            ts_log[b] += out.time[out.tx_off[b]:out.tx_off[b + 1]].tolist()
            pos[b] += int(K[b])
            call[b] += 1
    for b, g in enumerate(fx):
        assert np.array_equal(hb.rounds(b), g["round"]) and np.array_equal(hb.can_see(b), g["can_see"])
        wit = hb.witnesses(b)
        assert np.array_equal(wit, g["witnesses"])
        assert np.array_equal(hb.famous_events(b), g["famous"]) and np.array_equal(hb.consensus(b), g["consensus"])
        tx = hb.transactions(b)
        assert np.array_equal(tx, g["transactions"])
        assert rr_log[b] == g["asis_round_received"][tx].tolist() and same_bits(np.array(ts_log[b]), g["asis_consensus_time"][tx])
        if period == 1:
            assert len(tx) == 0 and not hb.consensus(b).any() and (hb.famous_events(b) == -1).all()
    for i, rec in enumerate(records):
        batch_assert_same(rec.o, hb, len(fx) + i)
    hb.close()


# ---- f. the partitioned decide_fame, and linking contexts of different periods --------------------------------------------------
@pytest.mark.parametrize("shape,nparts", [("n40", 2), ("n65", 3), ("n130", 2), ("n256", 3)])
def test_partitioned_fame_at_period_2(pkg, oracle_runs, shape, nparts):
    """tests/test_gpu_partition.py's check on section b's period-2 cases: every part runs its share of the elections, the
    element-wise maximum of their tables is committed on each."""
    part = importlib.import_module("py-swirld_amd.partition")
    run = oracle_runs.get(pool_name(shape, 2, False))
    o = run.oracle
    co = o.counters()
    assert co["coin_votes"] > 0 and 0 < co["coin_flips"] < co["coin_votes"]
    parts = [pkg.Hashgraph(run.n, coin_period=2) for _ in range(nparts)]
    for h in parts:
        h.append_events(*run.stream)
        h.divide_rounds(0, run.N)
    tables = [h.decide_fame_partial(p, nparts) for p, h in enumerate(parts)]
    fam, dec = part.merge_fame_tables(tables)
    wit = o.witnesses()
    m = wit >= 0
    coin = 0
    for h in parts:
        assert [int(r) for r in h.commit_fame(fam, dec)] == run.new_c
        assert np.array_equal(h.famous()[m], o.famous_by_event[wit[m]])
        assert np.array_equal(h.consensus(), o.consensus())
        coin += h.counters()["coin_votes"]
        h.close()
    assert coin == co["coin_votes"], "the parts' shares of the coin votes add up to the whole"


def test_split_link_refuses_contexts_of_different_periods(pkg):
    a, b, c = pkg.Hashgraph(8, coin_period=2), pkg.Hashgraph(8, coin_period=3), pkg.Hashgraph(8, coin_period=2)
    with pytest.raises(pkg.SwirldHipError) as ei:
        pkg.Hashgraph.split_link([a, b])
    assert ei.value.code == -22 and "same hashgraph" in str(ei.value)
    pkg.Hashgraph.split_link([a, c])     # the same period links
    a.split_unlink()
    for h in (a, b, c):
        h.close()


# ---- g. degenerate periods ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n4_s1_batch_c1", "n7_s2_chunk13_c1"])
def test_period_1_decides_nothing_and_votes_to_the_full_depth(pkg, name):
    g = cp.load(name)
    h = pkg.Hashgraph(g["n"], g["stake"], coin_period=1)
    o = Oracle(g["n"], g["stake"], 1)
    for a, b in g["batches"]:
        for d in (h, o):
            d.append_events(*slices(g, a, b))
            d.divide_rounds(a, b - a)
        assert len(h.decide_fame()) == 0 and len(o.decide_fame()) == 0
        assert len(h.find_order([])) == 0
    R = g["witnesses"].shape[0]
    assert (h.famous() == -1).all() and not h.consensus().any() and h.num_ordered == 0
    c, co = h.counters(), o.counters()
    assert {k: c[k] for k in FAME_COUNTERS} == {k: co[k] for k in FAME_COUNTERS}
    assert co["coin_votes"] == co["majority_evals"] > 0 and co["max_vote_distance"] == R - 1 == g["max_vote_distance"], "every level is a coin round, down to the last"
    rnd = g["round"]
    deepest = g["votes"][(rnd[g["votes"][:, 0]] - rnd[g["votes"][:, 1]]) == R - 1]
    assert len(deepest) > 0, "round 0's witnesses are voted on by the last round's"
    check_votes_both_ways(h, g["votes"], g["witnesses"], rnd, g["creator"])
    h.close()


def test_a_period_beyond_the_rounds_is_the_run_at_6(pkg):
    """Wherever the oracle casts no coin vote at 6, periods 50 and 2^31 - 1 give the run at 6."""
    compared = 0
    for stream in ("n70_s3_batch_c2", "n10_s1_stake_c2", "n4_s1_batch_c2", "n16_s8_slow_c2", "n6_s3_stuck_stake_c2"):
        g = cp.load(stream)
        o6 = oracle_of(g, 6)
        if o6.counters()["coin_votes"] != 0:
            continue
        got = []
        for k in (6, 50, 2 ** 31 - 1):
            h = pkg.Hashgraph(g["n"], g["stake"], coin_period=k)
            ncs = []
            for a, b in g["batches"]:
                h.append_events(*slices(g, a, b))
                h.divide_rounds(a, b - a)
                ncs.append(h.decide_fame().tolist())
                ncs.append(h.find_order(ncs[-1]).tolist())
            got.append((ncs, h.rounds().tobytes(), h.famous().tobytes(), h.consensus().tobytes(), h.round_received().tobytes(),
                        h.consensus_time().tobytes(), as_set(h.votes_triples()), {x: h.counters()[x] for x in FAME_COUNTERS}))
            h.close()
        assert got[0] == got[1] == got[2], stream
        assert np.array_equal(np.frombuffer(got[0][1], np.int32), o6.round)
        compared += len(g["votes"]) > 0
    assert compared >= 1
    g = cp.load("n7_s2_chunk13_c50")          # ... and the reference itself at 50, where it casts none either
    assert g["coin_votes"] == 0
    h = pkg.Hashgraph(g["n"], g["stake"], coin_period=2 ** 31 - 1)
    run_fixture(h, g)
    assert as_set(h.votes_triples()) == as_set(g["votes"])
    h.close()


@pytest.mark.parametrize("period", [0, -3])
def test_periods_below_1_are_refused(pkg, period):
    with pytest.raises(pkg.SwirldHipError) as ei:
        pkg.Hashgraph(4, coin_period=period)
    assert ei.value.code == -22 and "coin_period" in str(ei.value)
    with pytest.raises(pkg.SwirldHipError) as ei:
        pkg.HashgraphBatch(2, 4, coin_period=period)
    assert ei.value.code == -22 and "coin_period" in str(ei.value)


def test_the_largest_period_is_accepted(pkg):
    pkg.Hashgraph(4, coin_period=2 ** 31 - 1).close()
    pkg.HashgraphBatch(2, 4, coin_period=2 ** 31 - 1).close()


# ---- h. Node and DeviceNetwork ------------------------------------------------------------------------------------------------------
def votes_by_id(o, ids):
    return {ids[y]: {ids[x]: bool(v) for y2, x, v in grp} for y, grp in _grouped(oracle_votes(o)).items()}


def _grouped(triples):
    out = {}
    for y, x, v in sorted(triples):
        out.setdefault(y, []).append((y, x, v))
    return out


def oracle_of_context(ids, hg, mindex, sched, period):
    """The oracle fed the events of one context in THAT context's order, on that context's call schedule (the first call
    is the root's divide_rounds, without decide_fame: swirld.py:75-80)."""
    index = {h: i for i, h in enumerate(ids)}
    N = len(ids)
    cr = np.array([mindex[hg[h].c] for h in ids], np.int32)
    sp = np.array([index[hg[h].p[0]] if hg[h].p else -1 for h in ids], np.int32)
    op = np.array([index[hg[h].p[1]] if hg[h].p else -1 for h in ids], np.int32)
    t = np.array([hg[h].t for h in ids], np.float64)
    sig = np.frombuffer(b"".join(hg[h].s for h in ids), np.uint8).reshape(N, 64)
    assert sum(sched) == N
    o, a = Oracle(len(mindex), None, period), 0
    for i, k in enumerate(sched):
        o.append_events(cr[a:a + k], sp[a:a + k], op[a:a + k], t[a:a + k], sig[a:a + k])
        o.divide_rounds(a, k)
        if i > 0:
            o.find_order(o.decide_fame())
        a += k
    return o


def test_device_network_with_period_3_equals_the_node_simulation(pkg, monkeypatch):
    """tests/test_gpu_votes.py's test_device_network_votes_equal_the_node_simulation with C = 3 in py-swirld_amd/node.py (the
    drop-in Node hands its module constant to its context) and DeviceNetwork(coin_period=3), at 300 turns.

    Events, rounds, the order and round received are equal between the two.  The votes are compared more strictly than
    with each other: each side's complete dict against the oracle at period 3 fed that side's own event order and call
    schedule, and the two sides' VALUES wherever both hold an entry.  Whether an entry EXISTS depends on the order in which
    a context registered its events (a voter behind the first decider of its round stores nothing, swirld.py:235, 263),
    and a Node adds a sync's events in another order than the device's payload ingest: measured here, 10 of 2 247 entries
    of two nodes at period 3 and 19 of 1 676 at period 6 exist on one side only, every one of them what the oracle gives
    for that side's order.  (The check at 6 runs 60 turns, where no such entry has appeared.)"""
    from test_gpu_turn import node_simulation
    node_mod = pkg.node
    monkeypatch.setattr(node_mod, "C", 3)
    sched = {}
    orig = node_mod.Node.divide_rounds

    def recording(self, events):
        events = tuple(events)
        sched.setdefault(id(self), []).append(len(events))
        return orig(self, events)
    monkeypatch.setattr(node_mod.Node, "divide_rounds", recording)
    n, turns = 4, 300
    seeds = [bytes([70 + n, m]) + bytes(30) for m in range(n)]
    payloads = lambda k: None if k % 2 == 0 else b"tx %d" % k   # noqa: E731
    nodes = node_simulation(pkg, seeds, turns, 20261020, payloads)
    rng = random.Random(20261020)
    clock = iter(range(1, 1 << 30))
    tick = lambda: 1.0e9 + 0.001 * next(clock)   # noqa: E731
    ev = node_mod.Event
    net = pkg.DeviceNetwork(seeds, event_class=(ev.__module__, ev.__qualname__), clock=tick, coin_period=3)
    worked = []
    turn = net.turn

    def recording_turn(i, j, payload, t):
        r = turn(i, j, payload, t)
        worked.append((i, r.n_stored))
        return r
    net.turn = recording_turn
    net.run(turns, rng.randrange, tick, payloads)
    # the same turns at the default period: another outcome, so a network that ignored its argument would not pass
    rng6, clock6 = random.Random(20261020), iter(range(1, 1 << 30))
    tick6 = lambda: 1.0e9 + 0.001 * next(clock6)   # noqa: E731
    at_6 = pkg.DeviceNetwork(seeds, event_class=(ev.__module__, ev.__qualname__), clock=tick6)
    at_6.run(turns, rng6.randrange, tick6, payloads)
    assert all(at_6.event_ids(i) == net.event_ids(i) for i in range(n)), "the gossip itself does not depend on the period"
    assert any(at_6.transactions(i) != net.transactions(i) or not np.array_equal(at_6.ctx[i].famous(), net.ctx[i].famous()) for i in range(n))
    at_6.close()
    common = coin_entries = 0
    for i, nd in enumerate(nodes):
        assert net.event_ids(i) == set(nd.hg) and len(nd.hg) > turns // n
        assert net.round(i) == {h: nd.round[h] for h in nd.hg}
        assert net.transactions(i) == list(nd.transactions)
        assert net.round_received(i) == {h: nd.round_received[h] for h in nd.transactions}
        of_node = {y: dict(nd.votes[y]) for y in nd.votes}
        of_node = {y: d for y, d in of_node.items() if d}
        of_net = net.votes(i)
        o_node = oracle_of_context(list(nd._ids), nd.hg, nd._mindex, sched[id(nd)], 3)
        o_net = oracle_of_context(net._ids(i), nd.hg, nd._mindex, [1] + [k + 1 for w, k in worked if w == i], 3)
        assert of_node == votes_by_id(o_node, list(nd._ids)), "the node's votes against the oracle on the node's order and schedule"
        assert of_net == votes_by_id(o_net, net._ids(i)), "the network's votes against the oracle on its own order and schedule"
        co = o_net.counters()
        assert co["coin_votes"] > 0 and 0 < co["coin_flips"] < co["coin_votes"], co
        both = [(y, x) for y in of_node for x in of_node[y] if x in of_net.get(y, {})]
        assert all(of_node[y][x] == of_net[y][x] for y, x in both)
        assert len(both) > 0.95 * max(sum(len(d) for d in of_node.values()), sum(len(d) for d in of_net.values()))
        common += len(both)
        coin_entries += sum(1 for y, x in both if nd.round[y] - nd.round[x] >= 3 and (nd.round[y] - nd.round[x]) % 3 == 0)
    assert common > 1000 and coin_entries > 100, "votes of coin rounds were among those compared"
    net.close()
