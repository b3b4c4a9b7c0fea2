"""GPU (-m gpu): what every subsystem of a context keeps or forgets across reset() and rewind() (include/swirld_hip.h states
the contract per subsystem; csrc/swirld_hip.hip: the rewind() / reset() of sw_ctx's state structs).  Checked differentially, with no
model: a context that was used and reset must be indistinguishable — bit for bit, on every getter and export — from a fresh one
with the same settings; a context that was rewound must read its ids, data and trunks as before, and after the same three
consensus calls every getter and export must repeat.  The settings (member keys, event class, signing keys) survive both."""
import numpy as np
import pytest

from test_exact_host import add_forks
from test_gpu_sign import keypairs, signer

pytestmark = pytest.mark.gpu

N_MEMBERS = 4
CLASS = ("lifecycle_state", "Event.Of.A.Test")


def universe(pkg, N, seed, kp):
    """golden_universe's dict (test_gpu_turn) for a synthetic stream: events, data of every shape None / empty / short, keys."""
    cr, sp, op, t, _ = pkg.synth_hashgraph(N_MEMBERS, N, seed)
    rng = np.random.default_rng(seed)
    d = [None if e % 3 == 0 else rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes() for e in range(N)]
    seeds, kps = kp
    return dict(n=N_MEMBERS, N=N, cr=cr.astype(np.int32), sp=sp.astype(np.int32), op=op.astype(np.int32), t=t.astype(np.float64), d=d,
                seeds=seeds, kps=kps)


@pytest.fixture(scope="module")
def streams(pkg):
    """Stream A (300 events) and stream B (200 events, another seed), each with the ids and signatures the device gives it."""
    kp = keypairs(pkg, N_MEMBERS, 61)
    out = []
    for N, seed in ((300, 61), (200, 62)):
        u = universe(pkg, N, seed, kp)
        h = fresh(pkg, u)
        _, u["ids"], u["sig"] = h.create_events(u["cr"], u["sp"], u["op"], u["t"], u["d"], want_ids=True)
        h.close()
        out.append(u)
    return out


def fresh(pkg, u):
    """A context with every setting made: member keys, signing seeds, event class."""
    h = signer(pkg, u["n"], u["seeds"], u["kps"])
    h.set_event_class(*CLASS)
    return h


ROUTES = ["create", "append"]


def feed(h, u, route):
    """The stream with ids, signatures and data — created on the device (the device append underneath), or appended from host
    arrays with set_event_ids and set_event_data behind — and taken through the three consensus calls."""
    if route == "create":
        first, ids, sig = h.create_events(u["cr"], u["sp"], u["op"], u["t"], u["d"], want_ids=True)
        assert first == 0 and np.array_equal(ids, u["ids"]) and np.array_equal(sig, u["sig"])
    else:
        h.append_events(u["cr"], u["sp"], u["op"], u["t"], u["sig"])
        h.set_event_ids(0, u["ids"])
        h.set_event_data(0, u["d"])
    assert h.num_events == u["N"]
    consensus_pass(h)
    return u["ids"]


def consensus_pass(h):
    h.divide_rounds(0, h.num_events)
    h.find_order(h.decide_fame())


def bits(v):
    if isinstance(v, dict):
        return {k: bits(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return [bits(x) for x in v]
    return (str(v.dtype), v.shape, v.tobytes()) if isinstance(v, np.ndarray) else v


def settings(h):
    keys, usable = h.member_keys()
    return bits(dict(keys=keys, usable=usable, event_class=h.event_class(), signing=h.signing_members()))


def stored(h):
    """What belongs to the events, not to the consensus calls."""
    return bits(dict(ids=h.event_ids(), data=h.get_event_data(), trunks=h.fork_trunks()))


def readings(h):
    """Every getter and export of the list, as comparable values (arrays by their bytes: NaNs and signed zeros included)."""
    head = h.num_events - 1
    r = dict(N=h.num_events, heights=h.heights(), rounds=h.rounds(), witnesses=h.witnesses(), famous=h.famous(), consensus=h.consensus(),
             transactions=h.transactions(), n_ordered=h.num_ordered, round_received=h.round_received(), consensus_time=h.consensus_time(),
             payload=h.export_payload(head, data=True), walk=h.export_walk(head, data=True), message=h.export_message(head))
    r = bits(r)
    r.update(stored(h))
    return r


def same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], k


@pytest.mark.parametrize("route_a,route_b", [(a, b) for a in ROUTES for b in ROUTES])
def test_reset_leaves_a_fresh_context_with_its_settings(pkg, streams, route_a, route_b):
    """route_a then route_b: a device append leaves heights on the device and a kernel behind the call, a host append leaves
    them to the host mirror — after a reset neither may show in the next stream's heights."""
    A, B = streams
    x = fresh(pkg, A)
    ids_a = feed(x, A, route_a)
    assert x.num_ordered > 0 and x.max_round >= 3
    x.fork_trunks()
    assert len(x.export_message(A["N"] - 1)) > 0
    kept = settings(x)
    x.reset()
    assert x.num_events == 0 and x.num_ordered == 0
    assert (x.lookup_event_ids(ids_a) == -1).all(), "an id of the forgotten events is still known"
    assert settings(x) == kept
    assert kept["signing"][2] == bytes([1] * N_MEMBERS) and kept["event_class"] == list(CLASS)
    y = fresh(pkg, B)
    feed(x, B, route_b)
    feed(y, B, route_b)
    assert y.num_ordered > 0
    same(readings(x), readings(y))
    assert settings(x) == kept == settings(y)
    x.close()
    y.close()


@pytest.mark.parametrize("route", ROUTES)
def test_rewind_keeps_the_events_and_repeats_the_consensus(pkg, streams, route):
    A, _ = streams
    x = fresh(pkg, A)
    feed(x, A, route)
    first, kept = readings(x), settings(x)
    assert first["n_ordered"] > 0
    x.rewind()
    assert x.num_events == A["N"] and x.num_ordered == 0
    same(stored(x), {k: first[k] for k in ("ids", "data", "trunks")})
    assert settings(x) == kept
    consensus_pass(x)
    same(readings(x), first)
    x.close()


def test_rewind_of_a_forked_hashgraph_repeats_its_votes(pkg):
    cr, sp, op, t, sig = add_forks(pkg.synth_hashgraph(N_MEMBERS, 150, 5), N_MEMBERS, 5, 3, start=40)
    h = pkg.Hashgraph(N_MEMBERS)
    h.set_exact_history(True)
    h.append_events(cr, sp, op, t, sig)
    assert h.exact

    def run():
        consensus_pass(h)
        return bits(dict(available=h.votes_available, votes=h.vote_entries(), rounds=h.rounds(), witnesses=h.witnesses(), famous=h.famous(),
                         consensus=h.consensus(), transactions=h.transactions(), round_received=h.round_received(),
                         consensus_time=h.consensus_time()))

    first = run()
    assert first["available"] and len(first["votes"][0][2]) > 0 and len(first["transactions"][2]) > 0
    h.rewind()
    assert h.exact and h.num_events == len(cr) and h.num_ordered == 0
    same(run(), first)
    h.close()
