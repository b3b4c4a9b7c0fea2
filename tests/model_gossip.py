"""Executable specification of the answering half of a sync (sw_get_known_heights[_device], sw_sync_diff,
sw_export_payload[_device]; include/swirld_hip.h, kernels in py-swirld_amd/csrc/gossip.hip.h) in numpy: what an event
sees, the heights an asker reports, the chain position ranges of the diff, and the slot order and slot contents of the
exported payload.  Works on a fork-free stream in topological order; never imported by the product."""
import numpy as np

import model_payload as mp


class Graph:
    """A stream (creator, self-parent, other-parent, t, sig by dense index) with the ids its events carry."""

    def __init__(self, n, cr, sp, op, t=None, sig=None, ids=None):
        self.n, self.N = int(n), len(cr)
        self.cr, self.sp, self.op = (np.asarray(a, np.int64) for a in (cr, sp, op))
        self.t = np.zeros(self.N, np.float64) if t is None else np.asarray(t, np.float64)
        self.sig = np.zeros((self.N, 64), np.uint8) if sig is None else np.asarray(sig, np.uint8).reshape(self.N, 64)
        if ids is None:
            ids = np.frombuffer(b"".join(mp.event_id(k) for k in range(self.N)), np.uint8).reshape(self.N, 32)
        self.ids = np.asarray(ids, np.uint8).reshape(self.N, 32)
        # height: 0 for a root, else 1 + the larger of the parents' (swirld.py:117-120)
        ht = [0] * self.N
        spl, opl = self.sp.tolist(), self.op.tolist()
        for e in range(self.N):
            if spl[e] >= 0:
                ht[e] = 1 + max(ht[spl[e]], ht[opl[e]])
        self.height = np.array(ht, np.int64)
        # every member's self-parent chain in chain order (= index order without forks) and each event's position in it
        self.chains = [np.flatnonzero(self.cr == m) for m in range(self.n)]
        self.seq = np.zeros(self.N, np.int64)
        for ch in self.chains:
            self.seq[ch] = np.arange(len(ch))
        self._spl, self._opl, self._crl = spl, opl, self.cr.tolist()

    def row(self, head):
        """can_see[head]: per member the newest event of that member among the ancestors-or-self of `head`, -1 none."""
        mark = bytearray(head + 1)
        mark[head] = 1
        row = [-1] * self.n
        spl, opl, crl = self._spl, self._opl, self._crl
        for e in range(head, -1, -1):
            if mark[e]:
                if row[crl[e]] < 0:
                    row[crl[e]] = e
                if spl[e] >= 0:
                    mark[spl[e]] = 1
                    mark[opl[e]] = 1
        return np.array(row, np.int64)

    def known_heights(self, head):
        """What Node.sync reports (swirld.py:125-126): the height of the newest event of every member `head` sees, -1 none."""
        row = self.row(head)
        return np.where(row >= 0, self.height[np.maximum(row, 0)], -1).astype(np.int32)

    def ranges(self, head, known=None):
        """(pos_first, pos_end): per member the chain positions [first, end) of the diff.  The end is one past the newest
        event of the member `head` sees; the start is the first position whose height exceeds the asker's (0 when the
        member is unknown to it: a negative height, or known None); the head itself is always in."""
        row = self.row(head)
        first, end = np.zeros(self.n, np.int64), np.zeros(self.n, np.int64)
        for m in range(self.n):
            if row[m] < 0:
                continue
            p1 = int(self.seq[row[m]]) + 1
            k = -1 if known is None else int(known[m])
            p0 = 0 if k < 0 else int(np.searchsorted(self.height[self.chains[m][:p1]], k, side="right"))
            if m == self.cr[head] and p0 >= p1:
                p0 = p1 - 1
            first[m], end[m] = p0, max(p0, p1)
        return first, end

    def export(self, head, known=None):
        """The payload: slots member-major, chain order inside a member.  A dict of the arrays of sw_export_payload."""
        first, end = self.ranges(head, known)
        ev = np.concatenate([self.chains[m][first[m]:end[m]] for m in range(self.n)]).astype(np.int64)
        sp, op = self.sp[ev], self.op[ev]
        zero = np.zeros((len(ev), 32), np.uint8)
        return dict(event=ev.astype(np.int32), ids=self.ids[ev],
                    sp_ids=np.where((sp >= 0)[:, None], self.ids[np.maximum(sp, 0)], zero),
                    op_ids=np.where((op >= 0)[:, None], self.ids[np.maximum(op, 0)], zero),
                    arity=np.where(sp >= 0, 2, 0).astype(np.uint8), creator=self.cr[ev].astype(np.int32),
                    t=self.t[ev], sig=self.sig[ev], first=first, end=end)
