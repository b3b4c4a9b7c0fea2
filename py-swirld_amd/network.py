"""The reference's test(n_nodes, n_turns) (swirld.py:331-345) with every node's view as a context of ONE GPU and every step
of a node (swirld.py:322-328) as one Hashgraph.gossip_turn: no event, id, signature or payload is built or held on the host.

Each context has the members' keys, the Event class, the signing seed of its OWN member only, a complete id index and a
complete data store, and its root made by create_event.  Read-outs are keyed by event id, as the reference's dicts are.
`Node` does not use this yet."""
import numpy as np

from . import crypto
from .engine import Hashgraph


class DeviceNetwork:
    def __init__(self, seeds, stake=None, device=0, event_class=("swirld", "Event"), clock=None, exact_history=False, coin_period=6):
        """seeds: one 32-byte Ed25519 seed per node, in member order.  clock: the roots' timestamps (default time.time).
        exact_history: every context keeps round received, consensus time and the votes (by event) once it has stored a
        forked event (Hashgraph.set_exact_history); round_received(i), consensus_time(i) and votes(i) then go on answering.
        coin_period: the reference's module constant C (swirld.py:17), as `Node` passes its own to its context."""
        from time import time
        clock = clock or time
        self.seeds = [bytes(s) for s in seeds]
        self.n = len(self.seeds)
        self.pks = [crypto.sign_seed_keypair(s)[0] for s in self.seeds]
        self._network = {pk: i for i, pk in enumerate(self.pks)}   # (the reference's network dict: {pk -> node})
        self.ctx = []
        self.heads = []          # per node: the dense index of its head in its own context
        self.results = []        # the TurnResult of every turn, in order
        for i in range(self.n):
            h = Hashgraph(self.n, stake, coin_period=coin_period, device=device)
            if exact_history:
                h.set_exact_history(True)
            h.set_member_keys(self.pks)
            h.set_event_class(*event_class)
            h.set_signing_seeds([i], [self.seeds[i]])
            self.heads.append(h.create_event(i, -1, -1, clock(), None))   # swirld.py:75-80
            h.divide_rounds(0, 1)
            self.ctx.append(h)

    def close(self):
        for h in self.ctx:
            h.close()
        self.ctx = []

    # ---- swirld.py:322-328 and 341-344
    def turn(self, i, j, payload, t):
        """Node i syncs with node j and creates its event with `payload` (bytes | None) at time t."""
        r = self.ctx[i].gossip_turn(self.ctx[j], i, self.heads[i], self.heads[j], t, payload, validate=True, data_store=True)
        if r.new_head >= 0:
            self.heads[i] = r.new_head
        self.results.append(r)
        return r

    def partner(self, i, randrange):
        """swirld.py:323, the expression itself — the order of a set of keys depends on how the set was built, and a dict's key
        view builds it its own way — on a network dict in member order."""
        c = tuple(self._network.keys() - {self.pks[i]})[randrange(self.n - 1)]
        return self._network[c]

    def run(self, n_turns, randrange, clock, payloads=None):
        """n_turns steps: the working node by randrange(n) (swirld.py:342), its partner as partner() picks it, the event's
        time from clock(), its payload from payloads(turn) (default None)."""
        for k in range(n_turns):
            i = randrange(self.n)
            j = self.partner(i, randrange)
            self.turn(i, j, payloads(k) if payloads else None, clock())
        return self

    # ---- read-outs of node i, keyed by event id
    def _ids(self, i):
        return [bytes(x) for x in self.ctx[i].event_ids()]

    def head(self, i):
        return bytes(self.ctx[i].event_ids(self.heads[i], 1)[0])

    def event_ids(self, i):
        return set(self._ids(i))

    def round(self, i):
        return dict(zip(self._ids(i), (int(r) for r in self.ctx[i].rounds())))

    def transactions(self, i):
        ids = self._ids(i)
        return [ids[e] for e in self.ctx[i].transactions()]

    def round_received(self, i):
        ids, rr = self._ids(i), self.ctx[i].round_received()
        return {ids[e]: int(rr[e]) for e in self.ctx[i].transactions()}

    def consensus_time(self, i):
        ids, ct = self._ids(i), self.ctx[i].consensus_time()
        return {ids[e]: float(ct[e]) for e in self.ctx[i].transactions()}

    def votes(self, i):
        """Node.votes of node i (swirld.py:60-61): {voter id: {candidate id: bool}}, the voters that hold an entry."""
        ids = self._ids(i)
        out = {}
        for y, x, v in self.ctx[i].votes_triples().tolist():
            out.setdefault(ids[y], {})[ids[x]] = bool(v)
        return out

    def ordered_data(self, i):
        """The data of the ordered events, in order (bytes | None)."""
        tx = self.ctx[i].transactions()
        if len(tx) == 0:
            return []
        return Hashgraph.unpack_data(*self.ctx[i].gather_event_data(np.asarray(tx, np.int32)))
