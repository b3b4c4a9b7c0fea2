"""Executable specification of answering a sync by the pruned walk (sw_sync_walk, sw_export_walk[_device],
sw_get_fork_trunks; include/swirld_hip.h, kernels in py-swirld_amd/csrc/walk.hip.h) in numpy / plain Python: the set the
reference's BFS reaches (swirld.py:154-161), its ascending list, the frontier widths of the level-synchronous walk, the slot
contents of the exported payload, and the trunk height of a forked member in two forms — the order-independent one the
kernel computes and the arrival-order one of Node._add_event_host.  Works on any stream in topological order, forks and
second roots included; never imported by the product."""
import numpy as np

import model_gossip as mg

NO_CAP = 2**31 - 1


class WalkGraph(mg.Graph):
    """model_gossip.Graph (heights, ids, slot contents) on a stream that may hold forks: `chains`, `seq`, `row` and `ranges`
    of the base class are meaningful only while it holds none."""

    def pruning(self, known=None, cap=None):
        """The height per member below which the walk does not descend: min(known, cap); negative = send everything."""
        k = np.full(self.n, -1, np.int64) if known is None else np.asarray(known, np.int64).copy()
        if cap is not None:
            k = np.minimum(k, np.asarray(cap, np.int64))
        return k.tolist()

    def levels(self, head, known=None, cap=None):
        """The BFS of swirld.py:154-161 from `head`, level by level: a list of lists of dense indices.  The head is level 0;
        a parent p of a reached event is reached iff pruning[creator(p)] < 0 or height(p) > pruning[creator(p)]; an event
        enters once, on the first level that reaches it."""
        prune = self.pruning(known, cap)
        sp, op, cr, ht = self._spl, self._opl, self._crl, self.height.tolist()
        seen = {head}
        out, cur = [], [head]
        while cur:
            out.append(cur)
            nxt = []
            for e in cur:
                for p in (sp[e], op[e]):
                    if p < 0 or p in seen:
                        continue
                    k = prune[cr[p]]
                    if k < 0 or ht[p] > k:
                        seen.add(p)
                        nxt.append(p)
            cur = nxt
        return out

    def walk(self, head, known=None, cap=None):
        """The ascending list of the walk's events (int32): what sw_sync_walk returns."""
        return np.array(sorted(e for lv in self.levels(head, known, cap) for e in lv), np.int32)

    def export_walk(self, head, known=None, cap=None):
        """The payload: slot s holds the s-th event in ascending dense index, contents as model_gossip.Graph.export."""
        return self.slots(self.walk(head, known, cap))

    def slots(self, events):
        ev = np.asarray(events, np.int64)
        sp, op = self.sp[ev], self.op[ev]
        zero = np.zeros((len(ev), 32), np.uint8)
        return dict(event=ev.astype(np.int32), ids=self.ids[ev],
                    sp_ids=np.where((sp >= 0)[:, None], self.ids[np.maximum(sp, 0)], zero),
                    op_ids=np.where((op >= 0)[:, None], self.ids[np.maximum(op, 0)], zero),
                    arity=np.where(sp >= 0, 2, 0).astype(np.uint8), creator=self.cr[ev].astype(np.int32),
                    t=self.t[ev], sig=self.sig[ev])

    def ancestors_heights(self, head):
        """known_heights for any stream: per member the LARGEST height among the ancestors-or-self of `head` (what
        can_see[head] yields without forks), -1 none."""
        out = [-1] * self.n
        for e in self.walk(head).tolist():
            out[self._crl[e]] = max(out[self._crl[e]], int(self.height[e]))
        return np.array(out, np.int32)

    # ---- the trunk height of a forked member
    def trunks(self, upto=None):
        """Order-independent: per member the smallest height among its events that are the self-parent of at least two
        events; -1 with at least two roots; NO_CAP if the member has not forked."""
        N = self.N if upto is None else upto
        children = [0] * N
        roots = [0] * self.n
        for e in range(N):
            if self._spl[e] >= 0:
                children[self._spl[e]] += 1
            else:
                roots[self._crl[e]] += 1
        out = [NO_CAP] * self.n
        for p in range(N):
            if children[p] >= 2:
                out[self._crl[p]] = min(out[self._crl[p]], int(self.height[p]))
        for c in range(self.n):
            if roots[c] >= 2:
                out[c] = -1
        return np.array(out, np.int32)

    def trunks_by_arrival(self, order=None):
        """Node._add_event_host's bookkeeping, events arriving in `order` (default: index order): an event whose self-parent
        is not the member's newest event so far is a fork, and lowers the member's trunk to its self-parent's height (-1
        for a second root)."""
        chain_head, trunk = {}, {}
        for e in (range(self.N) if order is None else order):
            c, s = self._crl[e], self._spl[e]
            if c in chain_head and chain_head[c] != (s if s >= 0 else None):
                th = int(self.height[s]) if s >= 0 else -1
                trunk[c] = min(trunk.get(c, th), th)
            chain_head[c] = e
        return np.array([trunk.get(c, NO_CAP) for c in range(self.n)], np.int32)


def arbitrary_heights(g, head, seed):
    """Heights no can_see row need yield: uniform in [-1, height(head) + 1] per member."""
    return np.random.default_rng(seed).integers(-1, int(g.height[head]) + 2, g.n).astype(np.int32)


# (n, N, stream seed, head, heights seed) of fork-free streams from synth_hashgraph with arbitrary_heights.  On STRICT_CASE
# the walk names FEWER events than the chain ranges of sw_sync_diff (60 against 139): an event the asker lacks by height
# is reachable from the head only through events the asker reported knowing.
ARBITRARY_CASES = [(5, 300, 11, 299, 1), (33, 1500, 12, 750, 2), (33, 1500, 12, 1499, 3), (70, 2500, 13, 1250, 4), (130, 3000, 14, 2999, 5)]
STRICT_CASE = (33, 1500, 12, 750, 2)


def with_second_root(stream, member, seed):
    """The stream with one more event at its end: a second root of `member`, and an event of another member on top of it."""
    cr, sp, op, t, sig = stream
    rng = np.random.default_rng(seed)
    N = len(cr)
    other = int((member + 1) % (int(cr.max()) + 1))
    last_other = int(np.flatnonzero(cr == other)[-1])
    extra = rng.integers(0, 256, (2, 64), dtype=np.uint8)
    return (np.concatenate([cr, [member, other]]).astype(np.int32), np.concatenate([sp, [-1, last_other]]).astype(np.int32),
            np.concatenate([op, [-1, N]]).astype(np.int32), np.concatenate([t, [t[-1] + 1, t[-1] + 2]]), np.concatenate([sig, extra]))


def ranges_set(g, head, known=None):
    """The events model_gossip's ranges name on a fork-free graph."""
    first, end = g.ranges(head, known)
    return set(int(e) for m in range(g.n) for e in g.chains[m][first[m]:end[m]])
