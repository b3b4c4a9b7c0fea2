"""Drop-in `Node` / `Event` with the reference's API (swirld.py:30, 36-328) whose virtual
voting — divide_rounds / decide_fame / find_order and the can_see reachability table they
sit on — runs on the GPU through the C-ABI (include/swirld_hip.h).

Same constructor, attribute names, method names, return values and call protocol as the
reference class, so code written against `swirld.Node` (its `main()` loop, `test()`, the
viz app that reads `round` / `famous` / `idx` / `height` / `hg`) keeps working:

    Node(kp, network, n_nodes, stake)               swirld.py:38
    new_event / is_valid_event / add_event           swirld.py:82-120   (host, unchanged role)
    sync / ask_sync                                  swirld.py:122-161  (host, unchanged role)
    divide_rounds(events) -> None                    swirld.py:187      -> sw_divide_rounds
    decide_fame() -> set of rounds                   swirld.py:224      -> sw_decide_fame
    find_order(new_c) -> None                        swirld.py:280      -> sw_find_order
    main() generator                                 swirld.py:315

State that the reference keeps in dicts keyed by 32-byte hashes lives in HBM keyed by dense
indices; `round`, `can_see`, `witnesses`, `famous` are lazy read-only Mapping views over it
(host glue keeps hash -> index and pk -> member maps).  The hot path has no CPU fallback.
"""
from collections import namedtuple
from collections.abc import Mapping
from pickle import dumps, loads
from time import time

import numpy as np

from . import crypto
from ._lib import SwirldHipError
from .engine import Hashgraph
from .hgutils import bfs, randrange, toposort

_pack_data, _unpack_data = Hashgraph.pack_data, Hashgraph.unpack_data   # (list of bytes | None <-> data, offsets, None flags)

C = 6  # coin-round period, swirld.py:17


def majority(it):
    """Stake-weighted vote tally; a tie counts as True (swirld.py:20-27)."""
    no = yes = 0
    for stake, vote in it:
        if vote:
            yes += stake
        else:
            no += stake
    return (False, no) if no > yes else (True, yes)


Event = namedtuple("Event", "d p t c s")  # payload, parents, time, creator pk, signature


def _wire_prefix(cls):
    """The first bytes of the canonical wire form of a sync reply under the event class `cls` (csrc/wire.hip.h)."""
    m, q = cls.__module__.encode("utf-8"), cls.__qualname__.encode("utf-8")
    return b"\x80\x04\x8c" + bytes([len(m)]) + m + b"\x8c" + bytes([len(q)]) + q + b"\x93\x940\x8e"


WIRE_PREFIX = _wire_prefix(Event)


class _RoundView(Mapping):
    """Node.round: {event hash -> round number} (swirld.py:51-52)."""

    def __init__(self, node):
        self._n = node

    def __getitem__(self, h):
        i = self._n._index[h]
        if i >= self._n._divided:
            raise KeyError(h)
        return int(self._n._rounds()[i])

    def __iter__(self):
        return iter(self._n._ids[: self._n._divided])

    def __len__(self):
        return self._n._divided


class _CanSeeView(Mapping):
    """Node.can_see: {event -> {member pk -> latest event of that member it sees}}
    (swirld.py:69-72); rows are fetched from HBM on demand."""

    def __init__(self, node):
        self._n = node

    def __getitem__(self, h):
        nd = self._n
        i = nd._index[h]
        if i >= nd._divided:
            raise KeyError(h)
        row = nd._dev.can_see(i, 1)[0]
        return {nd._members[c]: nd._ids[k] for c, k in enumerate(row) if k >= 0}

    def __iter__(self):
        return iter(self._n._ids[: self._n._divided])

    def __len__(self):
        return self._n._divided


class _WitnessView(Mapping):
    """Node.witnesses: {round -> {member pk -> witness hash}}; inner dicts are in
    registration order (ascending event index), which decide_fame relies on."""

    def __init__(self, node):
        self._n = node

    def _table(self):
        return self._n._witness_table()

    def __getitem__(self, r):
        tab = self._table()
        if not 0 <= r < tab.shape[0]:
            return {}  # the reference's defaultdict would create an empty dict
        row = tab[r]
        if self._n._dev.exact:  # forks: a sibling replaces a member's witness but keeps its dict position
            order = [int(c) for c in self._n._dev.witness_order(r)]
        else:
            order = [c for c in np.argsort(np.where(row >= 0, row, np.iinfo(np.int32).max), kind="stable") if row[c] >= 0]
        return {self._n._members[c]: self._n._ids[row[c]] for c in order}

    def __iter__(self):
        return iter(range(self._table().shape[0]))

    def __len__(self):
        return self._table().shape[0]


class _FamousView(Mapping):
    """Node.famous: {witness hash -> bool}, decided witnesses only (swirld.py:64, 263)."""

    def __init__(self, node):
        self._n = node

    def _dict(self):
        return self._n._famous_dict()

    def __getitem__(self, h):
        return self._dict()[h]

    def __iter__(self):
        return iter(self._dict())

    def __len__(self):
        return len(self._dict())


class _ConsensusView(Mapping):
    """Node.round_received / Node.consensus_time: {event hash -> round received (swirld.py:283) / consensus timestamp
    (swirld.py:305)} of exactly the events of Node.transactions, in that order.  The reference computes both inside
    find_order and drops them; here they stay on the device (csrc/consensus.hip.h).  On a context that stored a forked
    event (exact path) the view raises NotImplementedError with the library's message."""

    def __init__(self, node, which):
        self._n, self._k = node, which

    def __getitem__(self, h):
        vals = self._n._consensus_values()[self._k]
        return vals[self._n.idx[h]].item()      # (KeyError for an event that is not ordered, or not known)

    def __iter__(self):
        self._n._consensus_values()
        return iter(self._n.transactions)

    def __len__(self):
        self._n._consensus_values()
        return len(self._n.transactions)


class VotesUnavailable(LookupError):
    """Node.votes is not kept in this state: the context stored a forked event (the exact path keeps two
    vote layers, not the history: sw_get_vote -> SW_ENOTSUP) or fame was committed from a partitioned
    decide_fame (sw_commit_fame).  Deliberately NOT a KeyError: `votes.get(...)` / `in` must not read
    "no such entry" where the answer is unknown.  round / witnesses / famous / consensus are unaffected."""


class _VoterVotes(Mapping):
    """Node.votes[y]: {candidate witness hash -> bool} of one voter."""

    def __init__(self, node, y):
        self._n, self._y = node, y

    def _slot(self, h):
        nd = self._n
        e = nd._index[h]
        if e >= nd._divided:  # known event, not yet through divide_rounds: no round, hence no votes
            raise KeyError(h)
        return int(nd._rounds()[e]), nd._mindex[nd.hg[h].c]

    def _vote(self, rv, mv, rc, mc):
        # SW_ENOTSUP from sw_get_vote (exact path; fame committed from a partitioned decide_fame, whose deciding
        # voters are not recorded): "unknown", not "no such entry" 
        try:
            return self._n._dev.vote(rv, mv, rc, mc)
        except SwirldHipError as exc:
            if exc.code == -95:
                raise VotesUnavailable(str(exc)) from None
            raise

    def _entries(self):
        """exact_history on a context that stored a fork: this voter's {candidate index -> bool} from the store."""
        nd = self._n
        return nd._vote_entries().get(nd._index[self._y], {})

    def __getitem__(self, x):
        nd = self._n
        if nd._votes_by_event():
            if x not in nd._index:
                raise KeyError(x)
            return self._entries()[nd._index[x]]   # (KeyError: no entry)
        (rv, mv), (rc, mc) = self._slot(self._y), self._slot(x)
        wit = nd._witness_table()
        if wit[rv, mv] != nd._index[self._y] or wit[rc, mc] != nd._index[x]:
            raise KeyError(x)
        v = self._vote(rv, mv, rc, mc)
        if v < 0:
            raise KeyError(x)
        return bool(v)

    def __iter__(self):
        nd = self._n
        if nd._votes_by_event():
            yield from (nd._ids[x] for x in self._entries())
            return
        rv, mv = self._slot(self._y)
        wit = nd._witness_table()
        if not hasattr(nd._dev, "export_votes"):   # a backend without the bulk export: entry by entry
            for rc in range(rv):
                for mc in np.argsort(np.where(wit[rc] >= 0, wit[rc], np.iinfo(np.int32).max), kind="stable"):
                    if wit[rc, mc] >= 0 and self._vote(rv, mv, rc, int(mc)) >= 0:
                        yield nd._ids[wit[rc, mc]]
            return
        # the bulk route: the rows of y in the table of its voter round, candidate rounds ascending, the candidates of a
        # round in registration order (= ascending dense index)
        row_voter, row_cand, exists, _ = nd._votes_round(rv)
        y = nd._index[self._y]
        for i in range(np.searchsorted(row_voter, y, "left"), np.searchsorted(row_voter, y, "right")):
            rc = int(row_cand[i])
            mcs = np.flatnonzero(np.unpackbits(exists[i].astype("<u8").view(np.uint8), bitorder="little")[:wit.shape[1]])
            for e in np.sort(wit[rc, mcs]):
                yield nd._ids[e]

    def __len__(self):
        return sum(1 for _ in self)


class _VotesView(Mapping):
    """Node.votes: {voter witness -> {candidate witness -> bool}} (swirld.py:60-61).  The GPU
    elections keep votes as per-round member bitmasks; entries are recomputed on demand (one by
    sw_get_vote, a voter's whole dict from the table of its round, sw_export_votes) with the reference's full semantics, the decide_fame() call schedule included: a
    voter has an entry for every candidate it evaluated, in whichever call, before that candidate
    was decided (Appendix A Q8/Q9)."""

    def __init__(self, node):
        self._n = node

    def _check(self):
        if self._n._dev.exact and not self._n.exact_history:
            raise VotesUnavailable("votes are not kept once a forked event was stored (exact path)")

    def __getitem__(self, y):
        self._check()
        if y not in self._n._index:
            raise KeyError(y)
        return _VoterVotes(self._n, y)

    def __iter__(self):
        self._check()
        nd = self._n
        if nd._votes_by_event():   # the voters of the store, in its order (with forks a voter may have left the witness table)
            yield from (nd._ids[y] for y in nd._vote_entries())
            return
        wit = nd._witness_table()
        for r in range(1, wit.shape[0]):
            for m in np.argsort(np.where(wit[r] >= 0, wit[r], np.iinfo(np.int32).max), kind="stable"):
                if wit[r, m] >= 0:
                    yield nd._ids[wit[r, m]]

    def __len__(self):
        return sum(1 for _ in self)


class Node:
    # ask_sync from the device-resident state (sw_sync_diff) instead of the reference's
    # height-pruned BFS over Python dicts.  Same SET of events for honest askers; the reply dict is then
    # filled member by member instead of in BFS order, which changes nothing for the receiver except the
    # iteration order of a Python set (and with it the order concurrent events are added in) — so the
    # default keeps the BFS, which makes whole simulations reproduce the reference event for event.
    device_sync_diff = False
    # ask_sync by the height-pruned walk ON THE DEVICE (Hashgraph.sync_walk, csrc/walk.hip.h): the BFS of swirld.py:154-161
    # itself, with this node's trunk heights as the cap, so it also serves a context that has stored a fork (the exact path),
    # where device_sync_diff falls back to the host.  Exactly the BFS's SET for any heights; the reply dict is filled in
    # ascending dense index (a topological order) instead of BFS order.  Takes precedence over device_sync_diff.
    device_sync_walk = False
    # Batched is_valid_event crypto on the GPU (sw_crypto_verify_batch / sw_crypto_hash_batch, SURVEY.md
    # §8f N3) for sync payloads of at least this many events; smaller payloads go through libsodium on
    # the host (one signature costs a GPU thread ~1-2 ms of latency, a CPU core ~60 us).  None = never.
    device_crypto_threshold = 512
    # Whole sync payloads resolved, ordered, validated and appended on the GPU (sw_ingest_payload: the id index of the
    # context, csrc/resolve.hip.h) instead of toposort + one is_valid_event / add_event per event on the host, for payloads
    # of at least this many unknown events.  Only with accept_forks=True (the device call stores forks as the reference
    # does; dropping them is the host loop's job).  The stored SET is the host loop's; the order events are added in is
    # (acceptance wave, position in the payload) instead of the toposort's — both topological.  None = never.
    device_payload_threshold = None
    # The crypto of is_valid_event for a whole payload in ONE device call against the members' keys (sw_validate_payload: the
    # fixed-base table of csrc/validate.hip.h; signature by the creator's key AND id in one verdict), for payloads of at
    # least this many events; it then takes the place of the two stateless batches above.  The node hands its members' keys
    # to the context on first use.  None = never.
    device_validate_threshold = None
    # Event.d kept on the device beside the other fields (the data store of the context, csrc/data.hip.h).  False: every
    # route is as without it.  True: before every divide_rounds the context's store is caught up with the data of the
    # events it has not seen yet — the one place that covers every route by which events reach the device —, payloads
    # whose events carry bytes of at most 60 000 bytes take _batch_validate's array route too, and ordered_data() reads
    # the consensus stream's payloads back from the device.  An event whose d is neither None nor such bytes makes its
    # payload fall back to the host routes, and the store holds None for it: hg[h].d stays the truth for such events.
    device_data = False
    MAX_DEVICE_DATA = 60000
    # The body of a sync reply built and parsed on the device (Hashgraph.export_message / unpack_message, csrc/wire.hip.h)
    # instead of dumps((head, subset)) / loads(reply).  The canonical wire form is a pickle any peer's loads reads, so a
    # node with the switch on talks to nodes without it.  ask_sync: under device_sync_walk's precondition, and only while
    # every stored event has the shape the device can write (_is_plain_or_data) and the data store can be caught up
    # (device_data, or every d None); otherwise the call takes the routes below.  sync: a reply that starts with the
    # canonical header goes to the strict reader and NEVER to pickle.loads (a reply the reader refuses adds nothing); its
    # arrays take _batch_validate_plain's pack + validate and ingest_payload, and Event objects are built for the stored
    # events only.  Any other reply is unpickled as before.
    device_wire = False
    # What the reference keeps on a forked hashgraph beyond the order, kept here too (Hashgraph.set_exact_history,
    # csrc/exact_history.hip.h).  False: once this node has stored a fork, round_received / consensus_time raise
    # NotImplementedError, ordered_data() fails and votes raises VotesUnavailable.  True: the context is created with the
    # history; the three keep working after a stored fork, votes is then served by event from the context's store —
    # votes[y][x], `in`, iteration and len, voters and candidates in the store's order (not the reference's dict order) —
    # and VotesUnavailable is raised only when the store says so (its ceiling, a KeyError, no hand-over from the fast path).
    # The store is the reference's unbounded dict in device memory: a deployment opts in.
    exact_history = False

    def __init__(self, kp, network, n_nodes, stake, device=0, accept_forks=True):
        self.pk, self.sk = kp
        # Forked events (two events of a member on one self-parent; the reference stores them, README.md:84).
        # True [default]: stored as in the reference (swirld.py:104-112 has no fork detection); the device
        # context then moves to the exact path (csrc/exact.hip.h: identical results, one wavefront — a
        # Byzantine fork slows this node down, it does not stop it).  False: a forked event and everything
        # built on it is dropped in is_valid_event, which keeps the round-synchronous device path but cuts
        # this node off from every honest member that did accept the sibling (their later events have an
        # ancestor this node refuses) — only for closed simulations without equivocation.
        self.accept_forks = bool(accept_forks)
        self.network = network  # {pk -> Node.ask_sync}
        self.n = n_nodes
        self.stake = stake
        self.tot_stake = sum(stake.values())
        self.min_s = 2 * self.tot_stake / 3

        self.hg = {}          # {event hash -> Event}
        self.head = None
        self.tbd = set()      # events whose final order is not decided yet
        self.transactions = []
        self.idx = {}
        self.consensus = set()
        self.height = {}

        # dense indices for the device
        self._members = list(stake.keys())
        if len(self._members) != n_nodes:
            raise ValueError("stake must have one entry per member")
        self._mindex = {pk: i for i, pk in enumerate(self._members)}
        self._ids = []
        self._index = {}
        self._chain_head = {}  # {member pk -> its newest event in this view} (fork detection)
        self._trunk_height = {}  # {member pk that forked -> height of its earliest forked self-parent (-1: second root)}
        self._chains = [[] for _ in range(n_nodes)]  # per member: its events in self-parent order (hashes)
        self._pending = []    # (creator, self_parent, other_parent, t, sig) not yet uploaded
        self._uploaded = 0
        self._dev_ids = 0     # events whose id the device context knows (device_payload_threshold)
        self._dev_data = 0    # events whose data the device context holds (device_data)
        self._wire_checked = 0         # stored events judged for device_wire so far: those the device cannot write, those with data
        self._wire_unfit = 0
        self._wire_with_data = 0
        self._wire_replies = 0         # ask_sync replies built on the device; sync replies read by the strict reader
        self._wire_intakes = 0
        self._device_payloads = 0
        self._keys_on_device = False   # the context has the members' keys and the Event class (device_validate_threshold)
        self._plain_payloads = 0       # payloads whose signed bytes the device built (_batch_validate_plain)
        self._divided = 0
        self._device = device
        self._dev = Hashgraph(n_nodes, [stake[pk] for pk in self._members], coin_period=C, device=device)
        if self.exact_history:
            self._dev.set_exact_history(True)
        self._dev.set_forks(self.accept_forks)
        self._round_cache = np.zeros(0, np.int32)
        self._wit_cache = None
        self._fam_cache = None
        self._votes_cache = {}         # voter round -> its votes table (_votes_round)

        self.round = _RoundView(self)
        self.can_see = _CanSeeView(self)
        self.witnesses = _WitnessView(self)
        self.famous = _FamousView(self)
        self.votes = _VotesView(self)
        self._cons_cache = (np.zeros(0, np.int32), np.zeros(0, np.float64))
        self.round_received = _ConsensusView(self, 0)
        self.consensus_time = _ConsensusView(self, 1)

        # the node's own root event (swirld.py:75-80)
        h, ev = self.new_event(None, ())
        self.add_event(h, ev)
        self.divide_rounds((h,))
        self.head = h

    # ------------------------------------------------------------------ gossip side (host)
    def new_event(self, d, p):
        """Create, sign and hash a new event of this node (swirld.py:82-95)."""
        assert p == () or len(p) == 2
        assert p == () or self.hg[p[0]].c == self.pk   # first parent is the self-parent
        assert p == () or self.hg[p[1]].c != self.pk   # second parent is someone else's
        t = time()
        s = crypto.sign_detached(dumps((d, p, t, self.pk)), self.sk)
        ev = Event(d, p, t, self.pk, s)
        return crypto.generichash(dumps(ev)), ev

    def _signature_ok(self, ev):
        try:
            crypto.verify_detached(ev.s, dumps(ev[:-1]), ev.c)
            return True
        except ValueError:
            return False

    def _parents_ok(self, ev):
        if ev.p == ():
            return True
        if len(ev.p) != 2 or any(p not in self.hg for p in ev.p):
            return False
        mine, theirs = (self.hg[p].c for p in ev.p)
        return mine == ev.c and theirs != ev.c

    def _not_a_fork(self, h, ev):
        """DEVIATION from the reference (which has no fork detection, swirld.py:88-89, 110-112,
        README.md:84): an event whose self-parent is not its creator's newest event in this view
        (or a second root) is rejected, and with it everything built on top of it.  The device path
        needs one self-parent chain per member; dropping the fork keeps an honest node running
        where storing it would make every later divide_rounds fail."""
        if self.accept_forks or h in self.hg:  # (already accepted: sync re-validates the remote head, swirld.py:138)
            return True
        return self._chain_head.get(ev.c) == (ev.p[0] if ev.p else None)

    def is_valid_event(self, h, ev, _crypto=None):
        """Signature, hash and parent checks (swirld.py:97-108).  `_crypto` = (signature ok, event id)
        when both were precomputed by a device batch."""
        if _crypto is None:
            sig_ok, hid = self._signature_ok(ev), crypto.generichash(dumps(ev))
        else:
            sig_ok, hid = _crypto
        return bool(sig_ok) and hid == h and self._parents_ok(ev) and self._not_a_fork(h, ev)

    def _batch_crypto(self, eids, events):
        """{event id -> (signature ok, BLAKE2b-256 of the pickled event)} for a whole sync payload, on
        the GPU.  Malformed signatures / keys (wrong type or length) are simply invalid."""
        from .engine import hash_batch, verify_batch
        msgs, sigs, pks, whole, good = [], [], [], [], []
        for eid in eids:
            ev = events[eid]
            wf = isinstance(ev.s, (bytes, bytearray)) and len(ev.s) == 64 and isinstance(ev.c, (bytes, bytearray)) and len(ev.c) == 32
            good.append(wf)
            msgs.append(dumps(ev[:-1]))
            sigs.append(bytes(ev.s) if wf else b"\0" * 64)
            pks.append(bytes(ev.c) if wf else b"\0" * 32)
            whole.append(dumps(ev))
        ok = verify_batch(msgs, sigs, pks, device=self._device)
        ids = hash_batch(whole, device=self._device)
        return {eid: (bool(ok[i]) and good[i], ids[i]) for i, eid in enumerate(eids)}

    def _ensure_keys(self):
        """The context has the members' keys and the Event class from the first call on."""
        if not self._keys_on_device:
            self._dev.set_member_keys([bytes(pk) for pk in self._members])
            self._dev.set_event_class(Event.__module__, Event.__qualname__)
            self._keys_on_device = True

    def _batch_validate(self, eids, events):
        """{event id -> (valid, id)} for a whole sync payload from ONE device call (Hashgraph.validate_payload): valid =
        signed by its creator, a member, and hashing to its id.  dumps(ev[:-1]) and dumps(ev) are packed once; malformed
        events (wrong types or lengths) are simply invalid."""
        self._ensure_keys()
        if all(self._is_plain(eid, events[eid]) for eid in eids):
            return self._batch_validate_plain(eids, events)
        if self.device_data and all(self._is_plain_or_data(eid, events[eid]) for eid in eids):
            return self._batch_validate_plain(eids, events, with_data=True)
        is_b = lambda x, n: isinstance(x, (bytes, bytearray)) and len(x) == n
        msgs, whole, sigs, ids, good = [], [], [], [], []
        creator = np.full(len(eids), -1, np.int32)
        for i, eid in enumerate(eids):
            ev = events[eid]
            wf = is_b(ev.s, 64) and is_b(ev.c, 32) and is_b(eid, 32)
            good.append(wf)
            msgs.append(dumps(ev[:-1]))
            whole.append(dumps(ev))
            sigs.append(bytes(ev.s) if wf else b"\0" * 64)
            ids.append(bytes(eid) if wf else b"\0" * 32)
            if wf:
                creator[i] = self._mindex.get(bytes(ev.c), -1)
        ok = self._dev.validate_payload(msgs, np.frombuffer(b"".join(sigs), np.uint8), creator, whole=whole,
                                        ids=np.frombuffer(b"".join(ids), np.uint8))
        return {eid: ((True, eid) if ok[i] and good[i] else (False, None)) for i, eid in enumerate(eids)}

    @staticmethod
    def _is_plain(eid, ev):
        """True when dumps(ev[:-1]) and dumps(ev) are the fixed template Hashgraph.pack_events writes (csrc/pack.hip.h): an
        Event with data None, a float timestamp, parents () or two 32-byte ids, and creator key, signature and id of exactly
        type bytes and 32, 64 and 32 bytes.  No two fields may be ONE object: pickle would write the second as a memo read."""
        is_b = lambda x, n: type(x) is bytes and len(x) == n
        if type(ev) is not Event or ev.d is not None or type(ev.t) is not float or type(ev.p) is not tuple:
            return False
        if not (is_b(ev.c, 32) and is_b(ev.s, 64) and is_b(eid, 32)):
            return False
        if len(ev.p) == 0:
            return True
        return (len(ev.p) == 2 and is_b(ev.p[0], 32) and is_b(ev.p[1], 32)
                and ev.p[0] is not ev.p[1] and ev.p[0] is not ev.c and ev.p[1] is not ev.c)

    @classmethod
    def _is_plain_or_data(cls, eid, ev):
        """_is_plain, or the same shape with data of exactly type bytes and at most MAX_DEVICE_DATA bytes that is not the
        same object as another field (pickle would write a memo read): what pack_events writes with its data arguments."""
        if type(ev) is not Event:
            return False
        if ev.d is None:
            return cls._is_plain(eid, ev)
        if type(ev.d) is not bytes or len(ev.d) > cls.MAX_DEVICE_DATA or type(ev.p) is not tuple:
            return False
        if any(ev.d is x for x in (ev.c, ev.s) + ev.p):
            return False
        return cls._is_plain(eid, ev._replace(d=None))

    @classmethod
    def _storable_data(cls, d):
        """What the device store holds for an event with data d: d itself, or None where it cannot hold it."""
        return d if d is None or (type(d) is bytes and len(d) <= cls.MAX_DEVICE_DATA) else None

    @staticmethod
    def _payload_arrays(eids, events, mindex):
        """The arrays Hashgraph.pack_events / validate_payload take, for a payload of plain events: parents' ids, arity,
        creator (dense index, -1 for a non-member), timestamp, signature, id."""
        K = len(eids)
        evs = [events[eid] for eid in eids]
        zero = b"\0" * 32
        sp = np.frombuffer(b"".join(ev.p[0] if ev.p else zero for ev in evs), np.uint8).reshape(K, 32)
        op = np.frombuffer(b"".join(ev.p[1] if ev.p else zero for ev in evs), np.uint8).reshape(K, 32)
        arity = np.fromiter((len(ev.p) for ev in evs), np.uint8, K)
        creator = np.fromiter((mindex.get(ev.c, -1) for ev in evs), np.int32, K)
        t = np.fromiter((ev.t for ev in evs), np.float64, K)
        sig = np.frombuffer(b"".join(ev.s for ev in evs), np.uint8).reshape(K, 64)
        ids = np.frombuffer(b"".join(eids), np.uint8).reshape(K, 32)
        return sp, op, arity, creator, t, sig, ids

    def _batch_validate_plain(self, eids, events, with_data=False):
        """_batch_validate for plain events (_is_plain; with_data: _is_plain_or_data): no dumps per event — the arrays go to
        the device, which builds the signed bytes itself (Hashgraph.pack_events) and judges them
        (Hashgraph.validate_payload)."""
        sp, op, arity, creator, t, sig, ids = self._payload_arrays(eids, events, self._mindex)
        if with_data:
            data, data_off, data_none = _pack_data([events[eid].d for eid in eids])
            msgs, moff, whole, woff, enc = self._dev.pack_events(sp, op, arity, creator, t, sig, data=data, data_off=data_off, data_none=data_none)
        else:
            msgs, moff, whole, woff, enc = self._dev.pack_events(sp, op, arity, creator, t, sig)
        ok = self._dev.validate_payload((msgs, moff), sig, creator, whole=(whole, woff), ids=ids)
        self._plain_payloads += 1
        return {eid: ((True, eid) if ok[i] and enc[i] else (False, None)) for i, eid in enumerate(eids)}

    def _validate_threshold(self):
        """device_validate_threshold where the device verifier applies: real Ed25519 keys of 32 bytes."""
        if not crypto.HAVE_SODIUM or not all(isinstance(pk, (bytes, bytearray)) and len(pk) == 32 for pk in self._members):
            return None
        return self.device_validate_threshold

    def add_event(self, h, ev):
        """Store an event (swirld.py:114-120); it is uploaded with the next divide_rounds."""
        self._add_event_host(h, ev)
        sp, op = (self._index[ev.p[0]], self._index[ev.p[1]]) if ev.p else (-1, -1)
        self._pending.append((self._mindex[ev.c], sp, op, float(ev.t), ev.s))

    def _add_event_host(self, h, ev):
        """The host side of add_event: every dict and list of this view (the device side is _pending, or a payload call)."""
        self.hg[h] = ev
        if ev.c in self._chain_head and self._chain_head[ev.c] != (ev.p[0] if ev.p else None):
            # a fork of member ev.c: everything of it above the forked self-parent may be on a branch a peer lacks
            th = self.height[ev.p[0]] if ev.p else -1
            self._trunk_height[ev.c] = min(self._trunk_height.get(ev.c, th), th)
        self._chain_head[ev.c] = h
        self.tbd.add(h)
        self.height[h] = 1 + max(self.height[p] for p in ev.p) if ev.p else 0
        self._index[h] = len(self._ids)
        self._ids.append(h)
        self._chains[self._mindex[ev.c]].append(h)

    def _known_heights(self):
        """{member pk -> height of the newest event of that member my head can see}: what a
        peer needs to know to send only what I am missing (swirld.py:125-126)."""
        hd = self._index[self.head]
        if hd >= self._divided:
            raise KeyError(self.head)
        kh = self._dev.known_heights(hd)  # one device call: heights of the can_see[head] entries
        return {self._members[c]: int(v) for c, v in enumerate(kh) if v >= 0}

    def sync(self, pk, payload):
        """Pull-sync with `pk`; returns the new event ids in topological order
        (swirld.py:122-146)."""
        request = crypto.sign(dumps(self._known_heights()), self.sk)
        reply = crypto.sign_open(self.network[pk](self.pk, request), pk)
        if self.device_wire and bytes(reply[:len(WIRE_PREFIX)]) == WIRE_PREFIX:
            return self._sync_wire(bytes(reply), payload)
        remote_head, remote_hg = loads(reply)
        return self._sync_events(remote_head, remote_hg, payload)

    def _sync_events(self, remote_head, remote_hg, payload):
        """sync behind the reply's decoding: validate and store the unknown events of remote_hg, then the new event."""
        unknown = remote_hg.keys() - self.hg.keys()
        thr = self.device_crypto_threshold
        if not crypto.HAVE_SODIUM:  # stand-in signatures are keyed hashes: the device verifier (real Ed25519) would refuse all of them
            thr = None
        vthr = self._validate_threshold()
        dthr = self.device_payload_threshold
        if dthr is not None and self.accept_forks and len(unknown) >= max(dthr, 1):
            added = self._sync_payload_device(list(unknown), remote_hg, thr, vthr)
            return self._sync_finish(added, remote_head, remote_hg, payload)
        new = tuple(toposort(unknown, lambda u: remote_hg[u].p))
        if vthr is not None and len(new) >= max(vthr, 1):
            pre = self._batch_validate(new, remote_hg)
        else:
            pre = self._batch_crypto(new, remote_hg) if thr is not None and len(new) >= thr else {}
        # Only what was actually stored is returned (main() hands it to divide_rounds): the reference
        # returns the rejected ids too and then fails on them (swirld.py:134-146, 326), and references an
        # unbound `h` when the remote head itself is rejected; here a bad payload costs the step, not the node.
        added = []
        for eid in new:
            if self.is_valid_event(eid, remote_hg[eid], pre.get(eid)):
                self.add_event(eid, remote_hg[eid])
                added.append(eid)
        return self._sync_finish(added, remote_head, remote_hg, payload)

    def _sync_payload_device(self, eids, remote_hg, crypto_thr, validate_thr=None):
        """The unknown events of a sync payload, in any order, through Hashgraph.ingest_payload; returns the ids stored,
        in the order they were added."""
        self._catch_up_ids()
        is32 = lambda x: isinstance(x, (bytes, bytearray)) and len(x) == 32
        eids = [e for e in eids if is32(e)]   # (anything else cannot be the BLAKE2b-256 of an event)
        K = len(eids)
        if K == 0:
            return []
        if validate_thr is not None and K >= validate_thr:
            pre = self._batch_validate(eids, remote_hg)
        else:
            pre = self._batch_crypto(eids, remote_hg) if crypto_thr is not None and K >= crypto_thr else None
        ids = np.frombuffer(b"".join(bytes(e) for e in eids), np.uint8).reshape(K, 32)
        par = np.zeros((2, K, 32), np.uint8)
        arity = np.zeros(K, np.uint8)
        creator = np.full(K, -1, np.int32)
        ok = np.zeros(K, np.uint8)
        t = np.zeros(K, np.float64)
        sig = np.zeros((K, 64), np.uint8)
        for i, eid in enumerate(eids):
            ev = remote_hg[eid]
            try:
                good = isinstance(ev.p, tuple) and all(is32(p) for p in ev.p) and isinstance(ev.s, (bytes, bytearray)) and len(ev.s) == 64
                if good:
                    t[i] = float(ev.t)
                    sig[i] = np.frombuffer(bytes(ev.s), np.uint8)
                    arity[i] = min(len(ev.p), 255)
                    if len(ev.p) == 2:
                        par[0, i] = np.frombuffer(bytes(ev.p[0]), np.uint8)
                        par[1, i] = np.frombuffer(bytes(ev.p[1]), np.uint8)
                    creator[i] = self._mindex.get(ev.c, -1)
                    sig_ok, hid = pre[eid] if pre is not None else (self._signature_ok(ev), crypto.generichash(dumps(ev)))
                    ok[i] = bool(sig_ok) and hid == eid
            except Exception:  # noqa: BLE001  (a malformed event is an invalid event)
                ok[i] = 0
        n_before = len(self._ids)
        out, n_stored = self._dev.ingest_payload(ids, par[0], par[1], arity, creator, ok, t, sig)
        self._device_payloads += 1
        added = []
        for j in np.argsort(out, kind="stable")[K - n_stored:] if n_stored else ():
            eid = eids[int(j)]
            assert out[j] == len(self._ids) >= n_before
            self._add_event_host(eid, remote_hg[eid])
            added.append(eid)
        self._uploaded += n_stored
        self._dev_ids = len(self._ids)
        return added

    def _catch_up_ids(self):
        """The context holds every stored event, and learns the ids of those added one by one since the last payload."""
        self._flush()
        if self._dev_ids < len(self._ids):
            self._dev.set_event_ids(self._dev_ids, np.frombuffer(b"".join(self._ids[self._dev_ids:]), np.uint8).reshape(-1, 32))
            self._dev_ids = len(self._ids)

    def _sync_wire(self, reply, payload):
        """sync for a reply in the canonical wire form (device_wire): the strict reader on the device, no unpickling."""
        self._ensure_keys()
        u = self._dev.unpack_message(reply)
        self._wire_intakes += 1
        if u is None:         # the canonical header in front of something the writer never writes: nothing is taken from it
            return ()
        remote_head = u["head"].tobytes()
        eids = [bytes(r) for r in u["ids"]]
        unknown = [i for i, e in enumerate(eids) if e not in self.hg]
        datas = _unpack_data(u["data"], u["data_off"], u["data_none"]) if not u["data_none"].all() else None

        def event(i):
            p = (u["sp_ids"][i].tobytes(), u["op_ids"][i].tobytes()) if u["arity"][i] else ()
            c = int(u["creator"][i])
            # (the key of no member: the event is invalid whatever stands here, and is never stored)
            return Event(None if datas is None else datas[i], p, float(u["t"][i]), self._members[c] if c >= 0 else b"", u["sig"][i].tobytes())

        remote_hg = {}
        if remote_head in self.hg:
            remote_hg[remote_head] = self.hg[remote_head]
        if not (self._validate_threshold() is not None and self.accept_forks and (self.device_data or datas is None)):
            # the array route does not apply: Event objects for the unknown events, then the host routes
            for i in unknown:
                remote_hg.setdefault(eids[i], event(i))
            return self._sync_events(remote_head, remote_hg, payload)
        added = []
        if unknown:
            self._catch_up_ids()
            self._catch_up_data()
            sel = np.asarray(unknown)
            ids, sp, op, arity, creator, t, sig = (np.ascontiguousarray(u[k][sel]) for k in ("ids", "sp_ids", "op_ids", "arity", "creator", "t", "sig"))
            kw = {}
            if datas is not None:
                lens = np.diff(u["data_off"])[sel]
                off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                src = np.repeat(u["data_off"][:-1][sel] - off[:-1], lens) + np.arange(int(off[-1]))
                kw = dict(data=np.ascontiguousarray(u["data"][src]), data_off=off, data_none=np.ascontiguousarray(u["data_none"][sel]))
            msgs, moff, whole, woff, enc = self._dev.pack_events(sp, op, arity, creator, t, sig, **kw)
            ok = self._dev.validate_payload((msgs, moff), sig, creator, whole=(whole, woff), ids=ids)
            self._plain_payloads += 1
            ok = (np.asarray(ok, bool) & np.asarray(enc, bool)).astype(np.uint8)
            out, n_stored = self._dev.ingest_payload(ids, sp, op, arity, creator, ok, t, sig, **(kw if self.device_data else {}))
            self._device_payloads += 1
            for j in np.argsort(out, kind="stable")[len(unknown) - n_stored:] if n_stored else ():
                i = unknown[int(j)]
                assert out[j] == len(self._ids)
                remote_hg[eids[i]] = event(i)
                self._add_event_host(eids[i], remote_hg[eids[i]])
                added.append(eids[i])
            self._uploaded += n_stored
            self._dev_ids = len(self._ids)
            if self.device_data:
                self._dev_data = len(self._ids)
        return self._sync_finish(added, remote_head, remote_hg, payload)

    def _sync_finish(self, added, remote_head, remote_hg, payload):
        if remote_head in remote_hg and self.is_valid_event(remote_head, remote_hg[remote_head]):
            h, ev = self.new_event(payload, (self.head, remote_head))
            assert self.is_valid_event(h, ev)
            self.add_event(h, ev)
            self.head = h
            added.append(h)
        return tuple(added)

    def ask_sync(self, pk, info):
        """Answer a sync request with every event the asker cannot know yet: walk back from
        my head, not descending below what the asker reported per member (swirld.py:148-161)."""
        asker_heights = loads(crypto.sign_open(info, pk))
        if ((self.device_wire or self.device_sync_walk) and self._index[self.head] < self._divided
                and all(isinstance(h, int) for h in asker_heights.values())):
            # the BFS below on the device (Hashgraph.sync_walk), trunk rule included; the reply holds the same events, in
            # ascending dense index instead of BFS order
            known = np.full(self.n, -1, np.int32)
            for creator, hgt in asker_heights.items():
                c = self._mindex.get(creator)
                if c is not None:
                    known[c] = min(hgt, 0x7FFFFFFF) if hgt >= 0 else -1
            cap = None
            if self._trunk_height:
                cap = np.full(self.n, 0x7FFFFFFF, np.int32)
                for creator, th in self._trunk_height.items():
                    cap[self._mindex[creator]] = th
            if self.device_wire and self._wire_ready():
                # ... and the reply's bytes with it (Hashgraph.export_message): no dict entry per event, no dumps
                self._wire_replies += 1
                return crypto.sign(self._dev.export_message(self._index[self.head], known, cap, data=self.device_data), self.sk)
        if (self.device_sync_walk and self._index[self.head] < self._divided
                and all(isinstance(h, int) for h in asker_heights.values())):
            subset = {}
            for i in self._dev.sync_walk(self._index[self.head], known, cap).tolist():
                subset[self._ids[i]] = self.hg[self._ids[i]]
            return crypto.sign(dumps((self.head, subset)), self.sk)
        # (a context on the exact path — it has stored a fork — has no sw_sync_diff and `_chains` is no longer
        # one chain per member: the BFS below serves it, so a peer cannot break ask_sync by delivering a fork)
        if self.device_sync_diff and not self._dev.exact and self._index[self.head] < self._divided:
            known = np.full(self.n, -1, np.int32)
            for creator, hgt in asker_heights.items():
                c = self._mindex.get(creator)
                if c is not None:
                    known[c] = min(int(hgt), 0x7FFFFFFF) if hgt >= 0 else -1
            first, end, _ = self._dev.sync_diff(self._index[self.head], known)
            subset = {self.head: self.hg[self.head]}
            for c in range(self.n):
                for eid in self._chains[c][first[c]:end[c]]:
                    subset[eid] = self.hg[eid]
            return crypto.sign(dumps((self.head, subset)), self.sk)

        # EXTENSION of the reference's height-pruned diff (swirld.py:154-161), active only for members this
        # node has seen fork: one reported height cannot tell which BRANCH the asker has (fork siblings
        # can even have equal heights), so for such a member the walk is pruned at its trunk — the part
        # below its earliest fork point, which every branch contains — instead of at the reported height.
        # Without it two honest nodes holding different siblings can never exchange them, and each
        # refuses everything the other builds afterwards (unknown parent).
        # COST: from the first fork of member c on, every answer re-sends c's events above the fork point to every
        # asker, for good (a second root: c's whole chain) — the asker drops what it already has, but pickling, signing and
        # transfer grow with c's history.  One equivocator therefore makes sync payloads O(history of that member); bounding
        # it needs the asker to report its branch tips for forked members (a protocol change the reference does not have).
        trunk = self._trunk_height

        def missing_parents(u):
            for p in self.hg[u].p:
                creator = self.hg[p].c
                known = asker_heights.get(creator)
                if known is not None and creator in trunk:
                    known = min(known, trunk[creator])
                if known is None or self.height[p] > known:
                    yield p

        subset = {}
        for eid in bfs((self.head,), missing_parents):
            subset[eid] = self.hg[eid]
        return crypto.sign(dumps((self.head, subset)), self.sk)

    def _wire_ready(self):
        """device_wire: every stored event is one the device can write, and ids, data store and keys are caught up."""
        if not all(type(pk) is bytes and len(pk) == 32 for pk in self._members):
            return False
        for h in self._ids[self._wire_checked:]:
            ev = self.hg[h]
            if not self._is_plain_or_data(h, ev):
                self._wire_unfit += 1
            elif ev.d is not None:
                self._wire_with_data += 1
        self._wire_checked = len(self._ids)
        if self._wire_unfit or (self._wire_with_data and not self.device_data):
            return False
        self._catch_up_ids()
        self._catch_up_data()
        self._ensure_keys()
        return True

    def ancestors(self, c):
        """Self-parent chain of c, newest first (swirld.py:163-168)."""
        while True:
            yield c
            if not self.hg[c].p:
                return
            c = self.hg[c].p[0]

    def higher(self, a, b):
        return a is not None and (b is None or self.height[a] >= self.height[b])

    def maxi(self, a, b):
        return a if self.higher(a, b) else b

    # ------------------------------------------------------------------ virtual voting (GPU)
    def _flush(self):
        if self._pending:
            cr, sp, op, t, sig = zip(*self._pending)
            self._dev.append_events(np.array(cr, np.int32), np.array(sp, np.int32), np.array(op, np.int32),
                                    np.array(t, np.float64),
                                    np.frombuffer(b"".join(sig), np.uint8).reshape(len(sig), 64))
            self._uploaded += len(self._pending)
            self._pending = []

    def _catch_up_data(self):
        """device_data: the context's data store learns the data of every event it has not seen yet, in one call."""
        first = self._dev_data
        if self.device_data and first < len(self._ids):
            self._dev.set_event_data(first, [self._storable_data(self.hg[h].d) for h in self._ids[first:]])
            self._dev_data = len(self._ids)

    def ordered_data(self, first=0, K=None):
        """[(event id, data)] of positions [first, first + K) of the consensus order (K None: to its end), the data read
        from the device in one export_ordered(..., data=True).  Needs device_data; an event whose d the store cannot hold
        (neither None nor bytes of at most MAX_DEVICE_DATA bytes) comes back as None."""
        if not self.device_data:
            raise RuntimeError("ordered_data needs Node.device_data = True")
        o = self._dev.export_ordered(first, K, data=True)
        datas = _unpack_data(o["data"], o["data_off"], o["data_none"])
        return [(self._ids[int(e)], d) for e, d in zip(o["event"], datas)]

    def divide_rounds(self, events):
        """Assign rounds / witnesses / can_see rows to the new events (swirld.py:187-222).
        `events` must be the not-yet-divided events in the order they were added (which is
        what sync() returns and main() passes)."""
        events = tuple(events)
        if not events:
            return
        first = self._divided
        expect = self._ids[first:first + len(events)]
        if list(events) != expect:
            for h in events:
                if h not in self.hg:
                    raise KeyError(h)
            raise ValueError("divide_rounds expects the undivided events in the order they were added")
        self._flush()
        self._catch_up_data()
        self._dev.divide_rounds(first, len(events))
        self._divided = first + len(events)
        self._wit_cache = None
        self._votes_cache = {}

    def decide_fame(self):
        """Run the witness elections; returns the set of newly decided rounds
        (swirld.py:224-277)."""
        new_c = {int(r) for r in self._dev.decide_fame()}
        self.consensus |= new_c
        self._fam_cache = None
        self._votes_cache = {}
        return new_c

    def find_order(self, new_c):
        """Extend the total order with the events the newly decided rounds receive
        (swirld.py:280-311)."""
        order = self._dev.find_order(new_c)
        final = [self._ids[i] for i in order]
        for i, x in enumerate(final):
            self.idx[x] = i + len(self.transactions)
        self.tbd.difference_update(final)
        self.transactions += final
        if self.consensus:
            print(self.consensus)

    def main(self):
        """Main working loop: `payload = yield new_event_ids` (swirld.py:315-328)."""
        new = ()
        while True:
            payload = (yield new)
            c = tuple(self.network.keys() - {self.pk})[randrange(self.n - 1)]
            new = self.sync(c, payload)
            self.divide_rounds(new)
            new_c = self.decide_fame()
            self.find_order(new_c)

    # ------------------------------------------------------------------ view plumbing
    def _rounds(self):
        have = self._round_cache.shape[0]
        if have < self._divided:
            self._round_cache = np.concatenate([self._round_cache, self._dev.rounds(have, self._divided - have)])
        return self._round_cache

    def _consensus_values(self):
        """(round received, consensus time) by position of Node.transactions; the positions added since the last look
        are fetched in one range of events."""
        if self._dev.exact and not self.exact_history:
            try:
                self._dev.round_received(0, 0)
            except SwirldHipError as exc:
                raise NotImplementedError(str(exc)) from None
            raise NotImplementedError("round received / consensus time are not kept on the exact (forked-hashgraph) path")
        have, n = self._cons_cache[0].shape[0], len(self.transactions)
        if have < n:
            ev = np.array([self._index[h] for h in self.transactions[have:]], np.int64)
            lo, hi = int(ev.min()), int(ev.max()) + 1
            rr, ct = self._dev.round_received(lo, hi - lo), self._dev.consensus_time(lo, hi - lo)
            self._cons_cache = (np.concatenate([self._cons_cache[0], rr[ev - lo]]), np.concatenate([self._cons_cache[1], ct[ev - lo]]))
        return self._cons_cache

    def _votes_by_event(self):
        return self.exact_history and self._dev.exact

    def _vote_entries(self):
        """exact_history on a context that stored a fork: {voter index -> {candidate index -> bool}} of the whole store
        (Hashgraph.vote_entries()), kept until the next divide_rounds or decide_fame."""
        t = self._votes_cache.get("entries")
        if t is None:
            try:
                y, x, v = self._dev.vote_entries()
            except SwirldHipError as exc:
                if exc.code == -95:
                    raise VotesUnavailable(str(exc)) from None
                raise
            t = {}
            for a, b, c in zip(y.tolist(), x.tolist(), v.tolist()):
                t.setdefault(a, {})[b] = bool(c)
            self._votes_cache["entries"] = t
        return t

    def _votes_round(self, rv):
        """The votes table of voter round rv (Hashgraph.export_votes(rv, rv + 1)), kept until the next divide_rounds or
        decide_fame.  A round decide_fame has not seen yet holds no votes."""
        t = self._votes_cache.get(rv)
        if t is None:
            try:
                t = self._dev.export_votes(rv, rv + 1)
            except SwirldHipError as exc:
                if exc.code == -95:
                    raise VotesUnavailable(str(exc)) from None
                if exc.code != -22:
                    raise
                nwo = (self.n + 63) // 64
                t = (np.empty(0, np.int32), np.empty(0, np.int32), np.empty((0, nwo), np.uint64), np.empty((0, nwo), np.uint64))
            self._votes_cache[rv] = t
        return t

    def _witness_table(self):
        if self._wit_cache is None:
            self._wit_cache = self._dev.witnesses()
        return self._wit_cache

    def _famous_dict(self):
        if self._fam_cache is None and self._dev.exact:
            # forks: a replaced witness keeps its entry (swirld.py:64 is keyed by event), so the per-event view
            fe = self._dev.famous_events(0, self._divided)
            self._fam_cache = {self._ids[int(e)]: bool(fe[e]) for e in np.flatnonzero(fe >= 0)}
        if self._fam_cache is None:
            wit, fam = self._witness_table(), self._dev.famous()
            d = {}
            for r in range(wit.shape[0]):
                row = wit[r]
                for c in np.argsort(np.where(row >= 0, row, np.iinfo(np.int32).max), kind="stable"):
                    if row[c] >= 0 and fam[r, c] >= 0:
                        d[self._ids[row[c]]] = bool(fam[r, c])
            self._fam_cache = d
        return self._fam_cache


def test(n_nodes, n_turns, device=0):
    """The reference's simulation driver (swirld.py:331-345): n_nodes nodes sharing an
    in-process 'network', stepped at random."""
    kps = [crypto.sign_keypair() for _ in range(n_nodes)]
    network = {}
    stake = {kp[0]: 1 for kp in kps}
    nodes = [Node(kp, network, n_nodes, stake, device=device) for kp in kps]
    for n in nodes:
        network[n.pk] = n.ask_sync
    mains = [n.main() for n in nodes]
    for m in mains:
        next(m)
    for i in range(n_turns):
        r = randrange(n_nodes)
        print("working node: %i, event number: %i" % (r, i))
        next(mains[r])
    return nodes
