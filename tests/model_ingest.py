"""CPU model of the device ingest (py-swirld_amd/csrc/ingest.hip.h), in the kernels' TILED form: local checks,
per-tile histograms + scan + stable in-tile rank (wave by wave, with running per-wave counts), link checks, and
heights by a per-tile fixed point.  Tile and wave sizes are parameters, so that a test can put every boundary
inside a small stream.  `sequential()` is the plain loop of the host path (sw_append_events, step 1) and of
ensure_dag_h, to compare against.  Never imported by the product.

Verdict: (event, code), the minimum over all offending events of (event << 8 | code) — what atomicMin leaves.
Why a clamped event cannot change the verdict: an event that fails a local check gets creator -1 and is left out
of the ranks.  The rank of an event counts EARLIER events of its creator only, so leaving event j out changes the
chain positions of events behind j and of no other; whatever the link checks then say about those events lies at
an index above j, and j itself is in the verdict already with a smaller word."""
import numpy as np

V_CREATOR, V_ARITY, V_ORDER, V_SELF, V_OTHER, V_FORK = 1, 2, 3, 4, 5, 6
NONE = None


class State:
    """What the context holds of the events so far: parent arrays, chain positions, heights, per-member tables."""

    def __init__(self, n):
        self.n = n
        self.cr = np.zeros(0, np.int32)
        self.sp = np.zeros(0, np.int32)
        self.op = np.zeros(0, np.int32)
        self.seq = np.zeros(0, np.int32)
        self.ht = np.zeros(0, np.int32)
        self.nev = np.zeros(n, np.int32)
        self.head = np.full(n, -1, np.int32)
        self.first = np.full(n, -1, np.int32)

    @property
    def N(self):
        return len(self.cr)


def _word(e, code):
    return (int(e) << 8) | code


def local_checks(cr, sp, op, first, n):
    """Step 1, one 'thread' per event: returns the clamped creators (-1 = takes part in nothing) and the verdict words."""
    key = cr.astype(np.int64).copy()
    words = []
    for i in range(len(cr)):
        e = first + i
        code = 0
        if cr[i] < 0 or cr[i] >= n:
            code = V_CREATOR
        elif (sp[i] < 0) != (op[i] < 0):
            code = V_ARITY
        elif sp[i] >= e or op[i] >= e:
            code = V_ORDER
        if code:
            key[i] = -1
            words.append(_word(e, code))
    return key, words


def tile_hist(key, first, n, tile, head, frst):
    """Step 2a: creators per tile; last / first event per member (atomicMax / atomicMin into the tables)."""
    K = len(key)
    tiles = (K + tile - 1) // tile
    hist = np.zeros((tiles, n), np.int64)
    head = head.astype(np.int64).copy()
    frst = np.where(frst >= 0, frst, 0x7fffffff).astype(np.int64)
    for t in range(tiles):
        for i in range(t * tile, min(K, (t + 1) * tile)):
            m = key[i]
            if m < 0:
                continue
            hist[t, m] += 1
            head[m] = max(head[m], first + i)
            frst[m] = min(frst[m], first + i)
    return hist, head, np.where(frst == 0x7fffffff, -1, frst)


def tile_scan(hist, nev):
    """Step 2b: exclusive scan over the tiles per member, from the member's count so far."""
    base = np.zeros_like(hist)
    run = nev.astype(np.int64).copy()
    for t in range(hist.shape[0]):
        base[t] = run
        run = run + hist[t]
    return base, run


def wave_peers(keys, valid, nbits):
    """Per lane: the set of lanes with an equal key, by ballots over the key's bits (as masks of Python ints)."""
    W = len(keys)
    full = sum(1 << l for l in range(W) if valid[l])
    peers = [full] * W
    for b in range(nbits):
        bal = sum(1 << l for l in range(W) if valid[l] and (keys[l] >> b) & 1)
        for l in range(W):
            peers[l] &= bal if (keys[l] >> b) & 1 else ~bal
    return peers


def tile_rank(key, base, n, tile, waves, wave):
    """Step 2c: every wave owns tile / waves consecutive events; counts of the waves in front give its base, then
    it walks its events `wave` at a time: rank = running count + popcount(peers in lower lanes)."""
    K = len(key)
    sub = tile // waves
    assert sub * waves == tile and sub % wave == 0
    nbits = max(1, int(np.ceil(np.log2(max(n, 2)))))
    seq = np.full(K, -1, np.int64)
    for t in range(base.shape[0]):
        wcnt = np.zeros((waves, n), np.int64)
        for w in range(waves):
            for i in range(t * tile + w * sub, min(K, t * tile + (w + 1) * sub)):
                if key[i] >= 0:
                    wcnt[w, key[i]] += 1
        run = base[t].copy()
        for w in range(waves):
            c = wcnt[w].copy()
            wcnt[w] = run
            run = run + c
        for w in range(waves):
            w0 = t * tile + w * sub
            for j in range(0, sub, wave):
                lanes = [w0 + j + l for l in range(wave)]
                keys = [int(key[i]) if i < K else -1 for i in lanes]
                valid = [k >= 0 for k in keys]
                peers = wave_peers(keys, valid, nbits)
                reads = [wcnt[w, keys[l]] if valid[l] else 0 for l in range(wave)]   # every read before any write
                for l in range(wave):
                    if not valid[l]:
                        continue
                    seq[lanes[l]] = reads[l] + bin(peers[l] & ((1 << l) - 1)).count("1")
                    if (peers[l] >> l) == 1:   # the highest lane of the group
                        wcnt[w, keys[l]] += bin(peers[l]).count("1")
    return seq


def link_checks(st, key, sp, op, seq_new, first):
    """Step 3, one 'thread' per event that passed step 1."""
    cr_all = np.concatenate([st.cr.astype(np.int64), key])
    seq_all = np.concatenate([st.seq.astype(np.int64), seq_new])
    words = []
    for i in range(len(key)):
        e, m = first + i, key[i]
        if m < 0:
            continue
        s, o = int(sp[i]), int(op[i])
        code = 0
        if s < 0:
            if seq_all[e] != 0:
                code = V_FORK
        elif cr_all[s] != m:
            code = V_SELF
        elif cr_all[o] == m:
            code = V_OTHER
        elif seq_all[s] + 1 != seq_all[e]:
            code = V_FORK
        if code:
            words.append(_word(e, code))
    return words


def heights_tiled(ht_old, sp, op, first, ht_tile):
    """Step 5: tiles in index order; parents in front of the tile are gathered, parents inside it resolved by a
    fixed point with at most `ht_tile` trips.  Returns (heights, most trips a tile needed, error flag)."""
    K = len(sp)
    ht = np.concatenate([ht_old.astype(np.int64), np.full(K, -1, np.int64)])
    worst = 0
    for t0 in range(0, K, ht_tile):
        tf = first + t0
        idx = range(t0, min(K, t0 + ht_tile))
        h = {}
        a, b = {}, {}
        for i in idx:
            s, o = int(sp[i]), int(op[i])
            if s < 0:
                h[i] = 0
                continue
            a[i] = ht[s] if s < tf else -1
            b[i] = ht[o] if o < tf else -1
            h[i] = 1 + max(a[i], b[i]) if a[i] >= 0 and b[i] >= 0 else -1
        trips = 0
        while any(h[i] < 0 for i in idx):
            trips += 1
            if trips > ht_tile:
                return ht[first:], worst, True
            snap = dict(h)   # every read of a trip before its writes
            for i in idx:
                if h[i] >= 0:
                    continue
                if a[i] < 0:
                    a[i] = snap[int(sp[i]) - first]
                if b[i] < 0:
                    b[i] = snap[int(op[i]) - first]
                if a[i] >= 0 and b[i] >= 0:
                    h[i] = 1 + max(a[i], b[i])
        worst = max(worst, trips)
        for i in idx:
            ht[first + i] = h[i]
    return ht[first:], worst, False


def block_spans(ht, first, shift=12):
    """[min, max] height per 2^shift-event block of the new events (what the level sweep's sizing reads)."""
    out = {}
    for i, h in enumerate(ht):
        b = (first + i) >> shift
        lo, hi = out.get(b, (0x7fffffff, -1))
        out[b] = (min(lo, int(h)), max(hi, int(h)))
    return out


def ingest(st, cr, sp, op, tile=16, waves=2, wave=4, ht_tile=8):
    """The device path for one batch.  Returns ((event, code) or None, new State or None): a verdict stores nothing."""
    cr, sp, op = (np.asarray(x, np.int64) for x in (cr, sp, op))
    first, n = st.N, st.n
    key, words = local_checks(cr, sp, op, first, n)
    hist, head, frst = tile_hist(key, first, n, tile, st.head, st.first)
    base, nev = tile_scan(hist, st.nev)
    seq = tile_rank(key, base, n, tile, waves, wave)
    words += link_checks(st, key, sp, op, seq, first)
    if words:
        w = min(words)
        return (w >> 8, w & 0xff), None
    ht, _, err = heights_tiled(st.ht, sp, op, first, ht_tile)
    assert not err
    new = State(n)
    new.cr = np.concatenate([st.cr, cr.astype(np.int32)])
    new.sp = np.concatenate([st.sp, sp.astype(np.int32)])
    new.op = np.concatenate([st.op, op.astype(np.int32)])
    new.seq = np.concatenate([st.seq, seq.astype(np.int32)])
    new.ht = np.concatenate([st.ht, ht.astype(np.int32)])
    new.nev, new.head, new.first = nev.astype(np.int32), head.astype(np.int32), frst.astype(np.int32)
    return None, new


def sequential(st, cr, sp, op):
    """The plain loop: per event, every check in the device path's order (local, self-parent's creator, other-parent's
    creator, fork); the first offending event ends it.  Returns ((event, code) or None, new State or None)."""
    n, first = st.n, st.N
    cr_all = list(st.cr) + [int(x) for x in cr]
    ht = list(st.ht)
    seq = list(st.seq)
    nev, head, frst = st.nev.copy(), st.head.copy(), st.first.copy()
    for i in range(len(cr)):
        e, m, s, o = first + i, int(cr[i]), int(sp[i]), int(op[i])
        if m < 0 or m >= n:
            return (e, V_CREATOR), None
        if (s < 0) != (o < 0):
            return (e, V_ARITY), None
        if s >= e or o >= e:
            return (e, V_ORDER), None
        if s >= 0 and cr_all[s] != m:
            return (e, V_SELF), None
        if o >= 0 and cr_all[o] == m:
            return (e, V_OTHER), None
        if head[m] != (s if s >= 0 else -1):
            return (e, V_FORK), None
        head[m] = e
        if frst[m] < 0:
            frst[m] = e
        seq.append(int(nev[m]))
        nev[m] += 1
        ht.append(0 if s < 0 else 1 + max(ht[s], ht[o]))
    new = State(n)
    new.cr = np.asarray(cr_all, np.int32)
    new.sp = np.concatenate([st.sp, np.asarray(sp, np.int32)])
    new.op = np.concatenate([st.op, np.asarray(op, np.int32)])
    new.seq, new.ht = np.asarray(seq, np.int32), np.asarray(ht, np.int32)
    new.nev, new.head, new.first = nev, head, frst
    return None, new
