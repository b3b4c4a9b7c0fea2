"""Executable specification of a payload call (sw_ingest_payload[_device], include/swirld_hip.h; kernels in
py-swirld_amd/csrc/resolve.hip.h) in plain Python: the status codes, the acceptance waves and the dense order.
`sequential()` is Node.sync's loop (swirld.py:130-136, node.py) over a toposorted payload with Node._parents_ok's
rules, to compare the accepted SET against.  Never imported by the product.

An event is a tuple (id, parent ids: () or a tuple of any length, creator, ok)."""
import hashlib

import numpy as np

DUP, NOT_OK, CREATOR, ARITY, PARENT, SELF, OTHER = -2, -3, -4, -5, -6, -7, -8


def event_id(k):
    """The id tests give the event with original index k."""
    return hashlib.blake2b(int(k).to_bytes(8, "little"), digest_size=32).digest()


class Index:
    """What the context holds: ids in dense order, their creators, id -> dense index."""

    def __init__(self, n):
        self.n = n
        self.ids = []
        self.cr = []
        self.of = {}

    def add(self, eid, creator):
        assert eid not in self.of
        self.of[eid] = len(self.ids)
        self.ids.append(eid)
        self.cr.append(int(creator))


def _local(index, events):
    """Known ids, duplicates, local checks and parent references: (out with None = candidate, refs of the candidates)."""
    K, n = len(events), index.n
    out = [None] * K
    lowest = {}
    for i, ev in enumerate(events):
        lowest.setdefault(ev[0], i)
    refs = {}
    for i, (eid, par, cr, ok) in enumerate(events):
        if eid in index.of:
            out[i] = index.of[eid]
        elif lowest[eid] != i:
            out[i] = DUP
        elif not ok:
            out[i] = NOT_OK
        elif not 0 <= cr < n:
            out[i] = CREATOR
        elif len(par) not in (0, 2):
            out[i] = ARITY
        else:
            r = []
            for p in par:
                if p in index.of:
                    r.append(("stored", index.of[p]))
                elif p in lowest:
                    r.append(("payload", lowest[p]))
                else:
                    out[i] = PARENT
            if out[i] is None:
                refs[i] = r
    return out, refs


def _creators_ok(index, events, i, refs):
    """None, or the reject code of a ready event."""
    if refs[i]:
        cs, co = (index.cr[x] if kind == "stored" else events[x][2] for kind, x in refs[i])
        if cs != events[i][2]:
            return SELF
        if co == events[i][2]:
            return OTHER
    return None


def _waves_literal(index, events, out, refs):
    """The waves as include/swirld_hip.h states them, wave by wave over the pending events (what the kernel does)."""
    wave = {}
    pending = sorted(refs)
    w = 0
    while True:
        accepted, rest = [], []
        for i in pending:
            if not all(kind == "stored" or (x in wave and wave[x] < w) for kind, x in refs[i]):
                rest.append(i)
                continue
            code = _creators_ok(index, events, i, refs)
            if code is None:
                accepted.append(i)
            else:
                out[i] = code
        for i in accepted:       # (after the wave: an event accepted in wave w is not a ready parent in wave w)
            wave[i] = w
        pending = rest
        if not accepted:
            return wave, w
        w += 1


def _waves_fast(index, events, out, refs):
    """The same waves in one pass: an event is decided once its payload parents are accepted, its wave is 1 + the
    largest of theirs (0 without any) — the wave in which the literal loop finds it ready for the first time."""
    children = {}
    missing = {}
    for i, r in refs.items():
        ps = {x for kind, x in r if kind == "payload"}
        missing[i] = len(ps)
        for x in ps:
            children.setdefault(x, []).append(i)
    wave = {}
    ready = [i for i in refs if missing[i] == 0]
    while ready:
        i = ready.pop()
        code = _creators_ok(index, events, i, refs)
        if code is not None:
            out[i] = code
            continue
        wave[i] = 1 + max((wave[x] for kind, x in refs[i] if kind == "payload"), default=-1)
        for ch in children.get(i, ()):
            missing[ch] -= 1
            if missing[ch] == 0:
                ready.append(ch)
    return wave, (1 + max(wave.values()) if wave else 0)


def ingest(index, events, commit=True, literal=False):
    """One payload call.  Returns (index_out: int array, order: payload positions in dense order, waves: accepting
    waves, parents: {position -> (dense sp, dense op) or (-1, -1)} of the accepted events)."""
    N0 = len(index.ids)
    out, refs = _local(index, events)
    wave, w = (_waves_literal if literal else _waves_fast)(index, events, out, refs)
    for i in refs:
        if i not in wave and out[i] is None:
            out[i] = PARENT     # never ready: a parent rejected, absent from both, or a cycle
    order = sorted(wave, key=lambda i: (wave[i], i))
    rank = {i: r for r, i in enumerate(order)}
    parents = {}
    for i in order:
        out[i] = N0 + rank[i]
        parents[i] = tuple(x if kind == "stored" else N0 + rank[x] for kind, x in refs[i]) or (-1, -1)
    if commit:
        for i in order:
            index.add(events[i][0], events[i][2])
    return np.array(out, np.int32), order, w, parents


def sequential(index, events, toposort):
    """The set of payload ids Node.sync's loop would store (accept_forks=True): unknown ids, toposorted, each checked
    with _parents_ok against what is stored by then.  The payload is a dict there: the lowest position of an id counts."""
    remote = {}
    for eid, par, cr, ok in events:
        remote.setdefault(eid, (par, cr, ok))
    have = dict(index.of)
    have_cr = {eid: index.cr[k] for eid, k in index.of.items()}
    unknown = [eid for eid in remote if eid not in have]
    unknown_set = set(unknown)
    stored = []
    try:
        order = list(toposort(unknown_set, lambda u: remote[u][0]))
    except ValueError:
        return None       # (a cycle: the reference's toposort gives up; the caller leaves such payloads to other checks)
    for eid in order:
        par, cr, ok = remote[eid]
        valid = bool(ok) and 0 <= cr < index.n
        if valid and par != ():
            valid = len(par) == 2 and all(p in have for p in par)
            if valid:
                valid = have_cr[par[0]] == cr and have_cr[par[1]] != cr
        if valid:
            have[eid] = len(have)
            have_cr[eid] = cr
            stored.append(eid)
    return stored


def from_stream(cr, sp, op, idx, id_of=event_id):
    """Payload events for the stream events `idx` (original indices), in that order."""
    return [(id_of(k), () if sp[k] < 0 else (id_of(sp[k]), id_of(op[k])), int(cr[k]), 1) for k in idx]


def to_arrays(events):
    """The arrays of the C-ABI: ids, sp_ids, op_ids (K x 32 uint8), arity (uint8), creator (int32), ok (uint8).  An arity
    other than 2 leaves the parent ids zero (they are ignored when it is 0, and the event is refused otherwise)."""
    K = len(events)
    ids = np.zeros((K, 32), np.uint8)
    spi = np.zeros((K, 32), np.uint8)
    opi = np.zeros((K, 32), np.uint8)
    ar = np.zeros(K, np.uint8)
    cr = np.zeros(K, np.int32)
    ok = np.zeros(K, np.uint8)
    for i, (eid, par, c, o) in enumerate(events):
        ids[i] = np.frombuffer(eid, np.uint8)
        ar[i] = len(par)
        if len(par) == 2:
            spi[i] = np.frombuffer(par[0], np.uint8)
            opi[i] = np.frombuffer(par[1], np.uint8)
        cr[i] = c
        ok[i] = o
    return ids, spi, opi, ar, cr, ok


def crafted_id(tag):
    return event_id(10_000_000 + tag)


def reject_payload(cr, sp, op, n, known, seed):
    """For a context that knows the first `known` events of the stream: a shuffled payload with the rest, 20 known ids,
    events of every reject code, a child and a grandchild of a rejected event and a 2-cycle.  Needs n >= 5.  Returns
    (events, expect) with expect = {payload position -> code} of the crafted events."""
    N = len(cr)
    rng = np.random.default_rng(seed)
    body = list(range(known, N)) + rng.choice(known, 20, replace=False).tolist()
    events = from_stream(cr, sp, op, body)
    X, E = crafted_id, event_id
    last = {int(cr[k]): k for k in range(N)}            # the newest event of every member
    crafted = [
        ((E(N - 1), (E(sp[N - 1]), E(op[N - 1])), int(cr[N - 1]), 1), DUP),
        ((X(1), (E(last[0]), E(last[1])), 0, 0), NOT_OK),
        ((X(2), (), n, 1), CREATOR),
        ((X(3), (), -1, 1), CREATOR),
        ((X(4), (E(last[0]),), 0, 1), ARITY),
        ((X(5), (E(last[0]), E(last[1]), E(last[2])), 0, 1), ARITY),
        ((X(6), (E(last[0]), X(999)), 0, 1), PARENT),                # an id that exists nowhere
        ((X(7), (E(last[1]), E(last[2])), 0, 1), SELF),
        ((X(8), (E(last[0]), E(sp[last[0]])), 0, 1), OTHER),
        ((X(9), (E(last[1]), X(7)), 1, 1), PARENT),                  # child of a rejected event
        ((X(10), (E(last[2]), X(9)), 2, 1), PARENT),                 # ... and its grandchild
        ((X(11), (E(last[3]), X(12)), 3, 1), PARENT),                # a 2-cycle
        ((X(12), (E(last[4]), X(11)), 4, 1), PARENT),
        ((X(13), (), n + 3, 0), NOT_OK),                             # several defects: the first in the order of the codes
        ((X(14), (E(last[0]),), n, 1), CREATOR),
        ((X(15), (E(last[1]), X(999)), 0, 1), PARENT),               # (a missing parent before a self-parent by another member)
    ]
    events += [ev for ev, _ in crafted]
    perm = rng.permutation(len(events)).tolist()
    # the in-payload duplicate AFTER the original (the lowest position counts)
    pos_dup, pos_orig = perm.index(len(body)), perm.index(body.index(N - 1))
    if pos_dup < pos_orig:
        perm[pos_dup], perm[pos_orig] = perm[pos_orig], perm[pos_dup]
    expect = {perm.index(len(body) + q): code for q, (_, code) in enumerate(crafted)}
    return [events[j] for j in perm], expect
