"""CPU: the drop-in `Node` (py-swirld_amd/node.py) against what the UNMODIFIED reference class computed, stored
under tests/golden/node/ by tests/golden/make_node_golden.py (which runs the reference where its tree is present).
Both sides are driven by their own `test(n_nodes, n_turns)` simulation (swirld.py:331-345) with the same random
bytes and the same clock.  The two runs gossip independently — sync payloads, height-pruned `ask_sync` subsets,
toposorted insertion, the sync event — and must end with the same hashgraph in every node: compared structurally
(an event = creator + position on its creator's chain).  Event hashes cover the pickled Event class, so both
sides hash a class-free serialisation here (see _class_free_dumps): the reference's results depend on the
insertion order of concurrent events, which follows the hashes.  The gossip partner is picked from a set of
bytes keys (swirld.py:322), so a simulation runs in a child process with a fixed hash seed, the seed the
reference ran under.  The device side of the drop-in is the CPU oracle here (tests/oracle_backend.py); the GPU
twin of the call protocol is tests/test_gpu_node.py.
"""
import contextlib
import gzip
import io
import json
import os
import pickle
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NODE_DIR = os.path.join(HERE, "golden", "node")
ROOT = os.path.dirname(HERE)
HASH_SEED = "0"
SIM_CASES = [(4, 250, 11), (5, 300, 12), (7, 900, 13), (3, 120, 14), (4, 600, 15), (6, 800, 16)]
FORK_CASES = [(4, 260, 31, 6), (5, 400, 32, 10), (3, 150, 33, 4)]


def _rng_bytes(seed):
    rng = random.Random(seed)
    return lambda k: bytes(rng.getrandbits(8) for _ in range(k))


def _clock():
    ticks = iter(range(1, 1 << 30))
    return lambda: 1.0e9 + 0.001 * next(ticks)


def _structure(node, members):
    """Everything a Node knows, keyed by (member index, position on that member's chain)."""
    mi = {pk: i for i, pk in enumerate(members)}
    key = {}
    for h, ev in node.hg.items():
        pos, cur = 0, ev
        while cur.p:
            pos += 1
            cur = node.hg[cur.p[0]]
        key[h] = (mi[ev.c], pos)
    parents = {key[h]: tuple(key[p] for p in ev.p) for h, ev in node.hg.items()}
    rounds = {key[h]: int(node.round[h]) for h in node.hg}
    wit = {int(r): {mi[pk]: key[h] for pk, h in d.items()} for r, d in node.witnesses.items() if d}
    famous = {key[h]: bool(v) for h, v in node.famous.items()}
    see_head = {mi[pk]: key[h] for pk, h in node.can_see[node.head].items()}
    return dict(head=key[node.head], parents=parents, rounds=rounds, witnesses=wit, famous=famous,
                consensus=sorted(int(r) for r in node.consensus), can_see_head=see_head,
                transactions=[key[h] for h in node.transactions], tbd=sorted(key[h] for h in node.tbd))


def canon(x):
    """JSON-able canonical form: dicts as key-sorted [key, value] pairs, tuples as lists, bytes as hex."""
    if isinstance(x, dict):
        return sorted([canon(k), canon(v)] for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return [canon(v) for v in x]
    if isinstance(x, (set, frozenset)):
        return sorted(canon(v) for v in x)
    if isinstance(x, bytes):
        return x.hex()
    return x


def _class_free_dumps(obj, *a, **k):
    """pickle.dumps, except that a top-level Event is serialised without its class path: the
    event hash (swirld.py:95) then is the same for swirld.Event and for the drop-in's Event, and
    with it everything that iterates containers keyed by hashes (toposort order = insertion order =
    witness registration order, which "first decider wins" depends on, swirld.py:235, 263)."""
    if hasattr(obj, "_fields"):
        obj = ("Event",) + tuple(obj)
    return pickle.dumps(obj, *a, **k)


def simulation_summary(nodes):
    members = [nd.pk for nd in nodes]
    return {"members": canon(members), "hg_sizes": [len(nd.hg) for nd in nodes],
            "nodes": [canon(_structure(nd, members)) for nd in nodes]}


def load(name):
    with gzip.open(os.path.join(NODE_DIR, name + ".json.gz"), "rt") as f:
        return json.load(f)


def _mirror_simulation(n, turns, seed):
    """The drop-in's own simulation (run in a child process: see the module docstring)."""
    import importlib
    sys.path[:0] = [ROOT, HERE]
    import oracle_backend
    pkg = importlib.import_module("py-swirld_amd")
    pkg.node.Hashgraph = oracle_backend.OracleHashgraph
    pkg.node.crypto.randombytes = _rng_bytes(seed)
    pkg.node.time = _clock()
    pkg.node.dumps = _class_free_dumps
    with contextlib.redirect_stdout(io.StringIO()):
        nodes = pkg.test(n, turns)
    return simulation_summary(nodes)


@pytest.mark.parametrize("n,turns,seed", SIM_CASES)
def test_simulation_matches_reference(pkg, n, turns, seed):
    ref = load("sim_%d_%d_%d" % (n, turns, seed))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), str(turns), str(seed)], capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, PYTHONHASHSEED=HASH_SEED))
    assert p.returncode == 0, p.stderr[-2000:]
    ours = json.loads(p.stdout.strip().splitlines()[-1])
    assert ref["members"] == ours["members"], "same random bytes must give the same key pairs"
    fields = ("head", "parents", "rounds", "witnesses", "famous", "consensus", "can_see_head", "tbd", "transactions")
    progressed = 0
    for a, b in zip(ref["nodes"], ours["nodes"]):
        a, b = dict(a), dict(b)
        for field in fields:
            assert a[field] == b[field], field   # (transactions: the total order, tie-breaks included)
        progressed += len(a["transactions"])
    assert len(ref["nodes"]) == len(ours["nodes"]) == n
    print("ordered events over all nodes:", progressed)
    assert all(s > turns // 4 for s in ref["hg_sizes"])


def test_is_valid_event_agrees_with_reference(pkg, monkeypatch):
    """N3, host side: the same accept / reject decisions as swirld.py:97-108 for
    well-formed events and for every way of malforming one (signature, hash, parents)."""
    import oracle_backend
    crypto = pkg.node.crypto
    want = dict(load("is_valid_event"))
    monkeypatch.setattr(pkg.node, "Hashgraph", oracle_backend.OracleHashgraph)
    monkeypatch.setattr(pkg.node, "dumps", _class_free_dumps)
    monkeypatch.setattr(pkg.node, "time", _clock())
    kps = [crypto.sign_seed_keypair(bytes([i]) * 32) for i in range(3)]
    stake = {kp[0]: 1 for kp in kps}
    ours = [pkg.Node(kp, {}, 3, stake) for kp in kps]
    for b in ours[1:]:  # give node 0 the roots of the others
        ours[0].add_event(b.head, b.hg[b.head])
    o0 = ours[0]
    good_h, good = o0.new_event(b"x", (o0.head, ours[1].head))
    cases = [("well-formed", good_h, good)]
    cases.append(("wrong hash", b"\0" * 32, good))
    cases.append(("tampered payload", good_h, good._replace(d=b"z")))
    cases.append(("tampered timestamp", good_h, good._replace(t=good.t + 1)))
    cases.append(("bad signature", good_h, good._replace(s=bytes(64))))

    def signed(p):
        ev = pkg.Event(b"x", p, good.t, o0.pk, b"")
        ev = ev._replace(s=crypto.sign_detached(_class_free_dumps(tuple(ev[:-1])), o0.sk))
        return crypto.generichash(_class_free_dumps(ev)), ev
    cases.append(("parents swapped (first is not the self-parent)",) + signed((ours[1].head, o0.head)))
    cases.append(("other-parent is mine",) + signed((o0.head, o0.head)))
    cases.append(("unknown parent",) + signed((o0.head, b"\x07" * 32)))
    cases.append(("one parent",) + signed((o0.head,)))
    assert sorted(name for name, _, _ in cases) == sorted(want)
    for name, h, ev in cases:
        assert o0.is_valid_event(h, ev) == want[name], name
    assert set(want.values()) == {True, False}


def forked_run(sign_keypair, n, steps, seed, n_forks, make_node):
    """The schedule of test_forked_hashgraph_matches_reference_node on one kind of Node: member 0 observes,
    everybody creates events, member n-1 forks.  Returns (observer, [(new_c, transactions) per call])."""
    kps = [sign_keypair(bytes([40 + i]) * 32) for i in range(n)]
    stake = {kp[0]: 1 for kp in kps}
    nodes = [make_node(kp, n, stake) for kp in kps]
    obs = nodes[0]
    rng = random.Random(seed)
    latest = {i: [nodes[i].head] for i in range(n)}      # per member: tips it may build on (two after a fork)
    pending = []
    for i in range(1, n):                                # the observer learns the other roots
        obs.add_event(nodes[i].head, nodes[i].hg[nodes[i].head])
        pending.append(nodes[i].head)
    for a in nodes:                                      # every creator knows every root (it signs on top of them)
        for i in range(n):
            if nodes[i].head not in a.hg:
                a.add_event(nodes[i].head, nodes[i].hg[nodes[i].head])
    fork_steps = set(rng.sample(range(10, steps - 10), n_forks))
    byz = n - 1
    calls = []

    def create(x, sp, op, payload):
        h, ev = nodes[x].new_event(payload, (sp, op))
        for nd in nodes:
            if h not in nd.hg:
                assert nd.is_valid_event(h, ev)
                nd.add_event(h, ev)
        pending.append(h)
        return h

    for step in range(steps):
        x = byz if step in fork_steps else rng.randrange(n)
        y = rng.choice([m for m in range(n) if m != x])
        sp = rng.choice(latest[x])
        op = rng.choice(latest[y])
        h1 = create(x, sp, op, b"p%d" % step)
        if step in fork_steps:                            # the sibling: same self-parent, another other-parent
            y2 = rng.choice([m for m in range(n) if m != x])
            h2 = create(x, sp, rng.choice(latest[y2]), b"q%d" % step)
            latest[x] = [h1, h2]
        else:
            latest[x] = [h1] if rng.random() < 0.7 else (latest[x] + [h1])[-2:]
        if step % 7 == 6 or step == steps - 1:            # the observer's main()-style call
            if latest[0][-1] in obs.hg:
                obs.head = latest[0][-1]
            obs.divide_rounds(list(pending))
            pending.clear()
            with contextlib.redirect_stdout(io.StringIO()):
                nc = obs.decide_fame()
                obs.find_order(nc)
            calls.append([canon(nc), canon(list(obs.transactions))])
    return obs, calls


def observer_state(obs):
    return {"round": canon({h: int(obs.round[h]) for h in obs.hg}),
            "witnesses": [[int(r), [[pk.hex(), h.hex()] for pk, h in d.items()]] for r, d in sorted(obs.witnesses.items()) if d],
            "famous": canon(dict(obs.famous.items())), "consensus": canon(set(obs.consensus)), "tbd": canon(set(obs.tbd)),
            "can_see_head": canon(dict(obs.can_see[obs.head])), "transactions": canon(list(obs.transactions)),
            "max_round": int(max(obs.round.values()))}


@pytest.mark.parametrize("n,steps,seed,n_forks", FORK_CASES)
def test_forked_hashgraph_matches_reference_node(pkg, monkeypatch, n, steps, seed, n_forks):
    """A Byzantine member forks (two events on one self-parent, later events on either sibling).  The
    unmodified reference class stores both (README.md:84); so does the drop-in with accept_forks=True —
    and an observer fed the same events in the same order and calling divide_rounds / decide_fame /
    find_order on the same schedule as the reference's must agree with it on every view: rounds,
    witnesses in dict order (a sibling replaces the value, not the position), fame, consensus,
    can_see of the head, the total order."""
    import oracle_backend
    ref = load("forked_%d_%d_%d_%d" % (n, steps, seed, n_forks))
    monkeypatch.setattr(pkg.node, "Hashgraph", oracle_backend.OracleHashgraph)
    monkeypatch.setattr(pkg.node, "dumps", _class_free_dumps)
    monkeypatch.setattr(pkg.node, "time", _clock())
    obs_o, calls = forked_run(pkg.node.crypto.sign_seed_keypair, n, steps, seed, n_forks,
                              lambda kp, n_, stake: pkg.Node(kp, {}, n_, stake, accept_forks=True))
    assert obs_o._dev.exact
    assert len(calls) == len(ref["calls"])
    for i, (a, b) in enumerate(zip(ref["calls"], calls)):
        assert a[0] == b[0], "new_c at call %d" % i
        assert a[1] == b[1], "total order at call %d" % i
    st = observer_state(obs_o)
    assert st["round"] == ref["state"]["round"]
    assert ref["state"]["max_round"] >= 3
    assert st["witnesses"] == ref["state"]["witnesses"], "witnesses, dict order included"
    assert st["famous"] == ref["state"]["famous"], "fame per event, replaced witnesses included"
    assert st["consensus"] == ref["state"]["consensus"] and st["tbd"] == ref["state"]["tbd"]
    assert st["can_see_head"] == ref["state"]["can_see_head"]
    assert st["transactions"] == ref["state"]["transactions"] and (len(st["transactions"]) > 0 or n == 3)


if __name__ == "__main__":   # the drop-in's simulation for test_simulation_matches_reference, in a child process
    print(json.dumps(_mirror_simulation(*[int(a) for a in sys.argv[1:4]])))
