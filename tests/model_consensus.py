"""Round received and consensus timestamp of an event in numpy: SURVEY.md Appendix A, Q10-Q12, written from that appendix
(fork-free hashgraphs).  Test scaffolding: the statement tests/test_model_consensus.py pins to the reference's own values
(tests/golden/consensus) and the GPU tests evaluate where no fixture exists.

Notation of the appendix: L[e][c] the final can_see row of e (event index, -1 = nothing of c), ht the heights, sp the
self-parents (-1 for a root), cr the creators, st the stakes with total T.

    Q10  find_order takes the rounds of each call in ascending order, call after call: `round_seq` is that sequence (the
         new_c of every call, sorted, one call behind the other).  An event still to be ordered is RECEIVED by the first
         round r of the sequence whose famous witnesses f_w satisfy 2 * sum(st[cr[w]] for w in s) > T with
         s = {w in f_w : L[w][cr[x]] != -1 and ht[L[w][cr[x]]] >= ht[x]}   (swirld.py:291-293, Q1: a strict float test).
         (Events the walk of swirld.py:288 cannot reach are not seen by any w either: what is ordered is closed under
         ancestry, so a path from w to x passes only events still to be ordered.)
    Q11  the sample of w in s: a = w; while a sees x (the test above on row a) and a is no root: a = sp[a]; sample t[a] —
         the first self-ancestor that does NOT see x, or the root.
    Q12  times sorted; ts = .5 * (times[len // 2] + times[(len + 1) // 2]); IndexError when len == 1.
"""
import numpy as np


def famous_table(wit, famous_by_event):
    """[R][n] fame of the witness slots (-1 no witness / undecided) from the per-event values of a golden."""
    wit = np.asarray(wit)
    return np.where(wit >= 0, np.asarray(famous_by_event)[np.maximum(wit, 0)], -1).astype(np.int8)


def consensus_values(events, round_seq, L, wit, fam, cr, sp, ht, t, stake, sample_lists=None):
    """(round_received, consensus_time) of `events` (dense indices, any order, no repeats): int32 with -1 and float64 with
    NaN where the event is not ordered by the rounds of `round_seq`.  `sample_lists` (a dict): filled with the sorted sample
    list of every ordered event, by event index."""
    events = np.asarray(events, np.int64)
    L, cr, sp, ht, t = np.asarray(L), np.asarray(cr), np.asarray(sp), np.asarray(ht), np.asarray(t, np.float64)
    st = np.asarray(stake, np.int64)
    T = int(st.sum())
    rr = np.full(len(events), -1, np.int32)
    cts = np.full(len(events), np.nan, np.float64)
    for r in round_seq:
        pend = np.flatnonzero(rr < 0)
        if len(pend) == 0:
            break
        row_w, row_f = np.asarray(wit[r]), np.asarray(fam[r])
        fw = row_w[(row_w >= 0) & (row_f == 1)].astype(np.int64)
        if len(fw) == 0:
            continue
        x = events[pend]
        k = L[fw[:, None], cr[x][None, :]]                              # [famous witness][pending event]
        sees = (k >= 0) & (ht[np.maximum(k, 0)] >= ht[x][None, :])
        got = 2 * (st[cr[fw]][:, None] * sees).sum(axis=0) > T
        if not got.any():
            continue
        wi, xi = np.nonzero(sees[:, got])                               # the (w, x) pairs that give a sample
        xs = x[got][xi]
        a = fw[wi].copy()
        while True:                                                      # Q11, every pair at once
            ka = L[a, cr[xs]]
            step = (ka >= 0) & (ht[np.maximum(ka, 0)] >= ht[xs]) & (sp[a] >= 0)
            if not step.any():
                break
            a = np.where(step, sp[a], a)
        by_x = np.argsort(xi, kind="stable")
        samples = t[a][by_x]
        end = np.cumsum(np.bincount(xi, minlength=int(got.sum())))
        for j, p in enumerate(pend[got]):
            times = np.sort(samples[end[j - 1] if j else 0:end[j]])
            if len(times) == 1:
                raise IndexError("event %d is seen by a single famous witness (swirld.py:305)" % events[p])
            rr[p] = r
            if sample_lists is not None:
                sample_lists[int(events[p])] = times
            cts[p] = .5 * (times[len(times) // 2] + times[(len(times) + 1) // 2])
    return rr, cts


def order_key_ok(tx, rr, cts):
    """(round received, consensus time) never decreases along a stretch of the order that ONE find_order call produced."""
    tx = np.asarray(tx)
    a, b = rr[tx], cts[tx]
    return bool(np.all((a[1:] > a[:-1]) | ((a[1:] == a[:-1]) & (b[1:] >= b[:-1]))))
