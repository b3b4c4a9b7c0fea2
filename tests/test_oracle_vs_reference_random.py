"""CPU: randomized differential test of the oracle against the UNMODIFIED reference — random member counts,
stakes, generator modes and call schedules.  What the reference computed for every case is
stored under tests/golden/random/ (tests/golden/make_random_golden.py records it where the reference tree is
present), inputs included, so the comparison runs anywhere."""
import os

import numpy as np
import pytest

from oracle.oracle import Oracle, OracleError

RANDOM_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random")


def random_case(rng):
    n = int(rng.integers(2, 28))
    N = int(rng.integers(n, 900))
    mode = int(rng.integers(0, 4))
    p0 = float(rng.uniform(0.01, 0.6))
    p1 = float(rng.uniform(0.005, 0.2))
    stake = None
    if rng.random() < 0.3:  # near-unit stakes still make progress (Appendix A Q2)
        stake = np.ones(n, np.int64)
        stake[rng.integers(0, n, size=max(1, n // 8))] = 2
    chunk = None if rng.random() < 0.5 else int(rng.integers(1, max(2, N // 3)))
    return n, N, mode, p0, p1, stake, chunk


def plain_case(synth, seed):
    """(n, stream, stake, chunk, lanes) of test_random_streams[seed]"""
    rng = np.random.default_rng(1000 + seed)
    n, N, mode, p0, p1, stake, chunk = random_case(rng)
    cr, sp, op, t, sig = synth(n, N, 5000 + seed, mode, p0, p1)
    t = t + rng.integers(0, 3, N) * 0.5  # ties and inversions in the timestamps
    return n, (cr, sp, op, t, sig), stake, chunk or N, None


def forked_case(synth, seed):
    """(n, stream, stake, chunk, lanes: the exact path's lane build) of test_random_forked_streams[seed]"""
    from test_exact_host import add_forks
    rng = np.random.default_rng(7000 + seed)
    n, N, mode, p0, p1, stake, chunk = random_case(rng)
    n, N = max(n, 3), max(N, 6 * n)
    base = synth(n, N, 9000 + seed, mode, p0, p1)
    stream = add_forks(base, n, seed, int(rng.integers(2, 30)))
    return n, stream, stake, chunk or len(stream[0]), bool(seed % 2) and (chunk is None or chunk > 30)


def load_case(kind, seed):
    with np.load(os.path.join(RANDOM_DIR, "%s_%02d.npz" % (kind, seed))) as z:
        g = {k: z[k] for k in z.files}
    stake = g["stake"] if len(g["stake"]) else None
    stream = (g["creator"], g["self_parent"], g["other_parent"], g["t"], g["sig"])
    calls = [(g["new_c_flat"][g["new_c_off"][i]:g["new_c_off"][i + 1]], g["tx_flat"][g["tx_off"][i]:g["tx_off"][i + 1]])
             for i in range(len(g["new_c_off"]) - 1)]
    wo = g["wit_order_flat"], g["wit_order_off"]
    g["wit_order"] = [wo[0][wo[1][r]:wo[1][r + 1]] for r in range(len(wo[1]) - 1)]
    return int(g["n"]), stream, stake, int(g["chunk"]), calls, int(g["index_error_call"]), g


@pytest.mark.parametrize("seed", range(24))
def test_random_streams(seed):
    n, (cr, sp, op, t, sig), stake, chunk, calls, index_error_call, ex = load_case("plain", seed)
    N = len(cr)
    orc = Oracle(n, None if stake is None else stake.astype(np.uint64))
    for i, a in enumerate(range(0, N, chunk)):
        b = min(N, a + chunk)
        orc.append_events(cr[a:b], sp[a:b], op[a:b], t[a:b], sig[a:b])
        orc.divide_rounds(a, b - a)
        nc_ref, tx_ref = calls[i]
        assert list(nc_ref) == list((nc := orc.decide_fame()))
        if i == index_error_call:  # swirld.py:305, single seeing witness (unequal stakes only)
            with pytest.raises(OracleError):
                orc.find_order(nc)
            return
        assert list(tx_ref) == list(orc.find_order(nc))
    assert np.array_equal(ex["round"], orc.round)
    assert np.array_equal(ex["can_see"], orc.can_see)
    assert np.array_equal(ex["witnesses"], orc.witnesses())
    assert np.array_equal(ex["famous"], orc.famous_by_event)
    assert np.array_equal(ex["consensus"], orc.consensus())
    assert np.array_equal(ex["transactions"], orc.transactions)
    assert int(ex["n_votes"]) == orc.num_votes


@pytest.mark.parametrize("seed", range(16))
def test_random_forked_streams(seed):
    """The same comparison on FORKED hashgraphs (the reference stores forks, README.md:84): height-based
    maxi with ties, witnesses replaced by fork siblings between calls, fame keyed by event, and — with
    them — the exact path's host builds next to the oracle."""
    from test_exact_host import ExactHost
    n, (cr, sp, op, t, sig), stake, chunk, calls, index_error_call, ex = load_case("forked", seed)
    N = len(cr)
    orc = Oracle(n, None if stake is None else stake.astype(np.uint64))
    exh = ExactHost(n, None if stake is None else stake.astype(np.uint32), lanes=bool(ex["lanes"]))
    for i, a in enumerate(range(0, N, chunk)):
        b = min(N, a + chunk)
        for d in (orc, exh):
            d.append_events(cr[a:b], sp[a:b], op[a:b], t[a:b], sig[a:b])
            d.divide_rounds(a, b - a)
        nc_ref, tx_ref = calls[i]
        assert list(nc_ref) == list((nc := orc.decide_fame())) == list(exh.decide_fame())
        if i == index_error_call:  # swirld.py:305
            with pytest.raises(OracleError):
                orc.find_order(nc)
            with pytest.raises(IndexError):
                exh.find_order(nc)
            return
        assert list(tx_ref) == list(orc.find_order(nc)) == list(exh.find_order(nc))
    st = exh.state()
    assert np.array_equal(ex["round"], orc.round) and np.array_equal(ex["round"], st["round"])
    assert np.array_equal(ex["can_see"], orc.can_see) and np.array_equal(ex["can_see"], st["can_see"])
    assert np.array_equal(ex["witnesses"], orc.witnesses()) and np.array_equal(ex["witnesses"], st["wit"])
    for r, order in enumerate(ex["wit_order"]):
        assert np.array_equal(order, orc.witness_order(r)) and np.array_equal(order, st["worder"][r])
    assert np.array_equal(ex["famous"], orc.famous_by_event) and np.array_equal(ex["famous"], st["fam"])
    assert np.array_equal(ex["consensus"], orc.consensus()) and np.array_equal(ex["consensus"], st["cons"])
    assert np.array_equal(ex["transactions"], orc.transactions)
    assert np.array_equal(ex["tbd"], orc.tbd) and np.array_equal(ex["tbd"], st["tbd"])
    assert int(ex["n_votes"]) == orc.num_votes
