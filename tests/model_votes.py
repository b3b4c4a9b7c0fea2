"""Specification of the votes table of sw_export_votes (include/swirld_hip.h; kernels in csrc/votes.hip.h) in numpy, from
the arrays a golden holds plus its call schedule: `witnesses`, `round`, the strongly-sees sets recomputed from `can_see`,
the coin bits from `sig`, the stake, `batches`, and the recorded new_c per decide_fame call.

Two independent halves, as in the comment above sw_get_vote:
  * the VALUE of votes[y][x] is a function of the hashgraph alone: the election of x replayed level by level, every
    witness voting (swirld.py:256-272);
  * whether the ENTRY exists follows from the decide_fame calls (swirld.py:224-277), which are replayed here one by one
    in the reference's own loop order — NOT by the closed rule (first / last call, deciding voter) the library uses, so
    that the two check each other.
The table: one row per (voter witness y, candidate round rc) with at least one entry, sorted by (round(y), y, rc);
exists / value as member bitmasks in ceil(n / 64) little-endian 64-bit words."""
import numpy as np

COIN_PERIOD = 6   # C of swirld.py; the default of the `coin_period` arguments below


def strongly_seen(g):
    """S[r, m] (r >= 1): bool[n], the members whose round r-1 witness the witness (r, m) strongly sees (swirld.py:247-254)."""
    wit, rnd, cs = g["witnesses"], g["round"], g["can_see"]
    stake = g["stake"].astype(np.int64)
    tot2 = 2 * int(stake.sum())
    R, n = wit.shape
    S = np.zeros((R, n, n), bool)
    for r in range(1, R):
        for m in range(n):
            y = wit[r, m]
            if y < 0:
                continue
            k = cs[y]                                           # per member c: the event of c that y sees
            via = (k >= 0) & (rnd[np.maximum(k, 0)] == r - 1)     # ... in round r - 1
            k2 = cs[k[via]]                                     # [via members][n]
            hit = (k2 >= 0) & (rnd[np.maximum(k2, 0)] == r - 1)
            hits = (hit * stake[via][:, None]).sum(axis=0)
            S[r, m] = 3 * hits > tot2
    return S


class Election:
    """The votes of every witness on the witnesses of round rc, level by level; level d is voter round rc + d."""

    def __init__(self, g, S, rc, coin_period=COIN_PERIOD):
        self.g, self.S, self.rc, self.coin_period = g, S, rc, int(coin_period)
        self.stake = g["stake"].astype(np.int64)
        self.tot2 = 2 * int(self.stake.sum())
        self.coin = g["sig"][:, 0] >> 7
        self.unit = bool((self.stake == 1).all())
        self.V, self.strong, self.coined, self.by_stake = [None], [None], [None], [None]

    def level(self, d):
        """(vote, supermajority, coin branch taken): bool [voter member][candidate member]; by_stake[d] beside them: the
        entries whose majority or supermajority by STAKE is not what a count of the same voters gives"""
        while len(self.V) <= d:
            k = len(self.V)
            wit = self.g["witnesses"][self.rc + k]
            has = wit >= 0
            Sk = self.S[self.rc + k] & has[:, None]
            if k == 1:
                self.V.append(Sk.copy())                           # x in s (swirld.py:258)
                self.strong.append(np.zeros_like(Sk))
                self.coined.append(np.zeros_like(Sk))
                self.by_stake.append(np.zeros_like(Sk))
                continue
            w = Sk * self.stake[None, :]                           # [voter][member]
            yes = w @ self.V[k - 1].astype(np.int64)               # [voter][candidate]
            no = w.sum(axis=1)[:, None] - yes
            vote = ~(no > yes)                                     # majority(): a tie is True (swirld.py:24-27)
            strong = 3 * np.where(vote, yes, no) > self.tot2
            by_stake = np.zeros_like(vote)
            if not self.unit:                                      # the same tally with every voter weighing 1, against 2 n / 3
                heads = Sk.astype(np.int64)
                yes_h = heads @ self.V[k - 1].astype(np.int64)
                no_h = heads.sum(axis=1)[:, None] - yes_h
                vote_h = ~(no_h > yes_h)
                strong_h = 3 * np.where(vote_h, yes_h, no_h) > 2 * len(self.stake)
                by_stake = ((vote != vote_h) | (strong != strong_h)) & has[:, None]
            self.by_stake.append(by_stake)
            coined = np.zeros_like(vote)
            if k % self.coin_period == 0:
                coined = ~strong & has[:, None]
                vote = np.where(strong, vote, self.coin[np.maximum(wit, 0)][:, None].astype(bool))   # swirld.py:272
            self.V.append(vote & has[:, None])
            self.strong.append(strong)
            self.coined.append(coined)
        return self.V[d], self.strong[d], self.coined[d]


def model_votes(g, new_c=None, coin_period=COIN_PERIOD):
    """-> dict(row_voter, row_cand_round, exists [rows][nwo] uint64, value, n_entries, n_coin, n_weighted, n_by_stake (the
    evaluated entries whose outcome by stake differs from a head count of the same voters), and the
    tables the library keeps beside the hashgraph: dec_call, dec_by, calls, cons_call, S).
    new_c: per call the rounds the reference put into `consensus` (default: the golden's record).
    coin_period: the reference's C for this run (default: its own, 6)."""
    wit, rnd = g["witnesses"], g["round"]
    R, n = wit.shape
    S = strongly_seen(g)
    if new_c is None:
        off = g["new_c_off"]
        new_c = [g["new_c_flat"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    unit = bool((g["stake"] == 1).all())
    elections = {}
    famous = np.zeros((R, n), bool)          # decided (the value itself plays no part in the votes)
    consensus = set()
    rows = {}                                # (y, rc) -> [exists bool[n], value bool[n]]
    dec_call = np.full((R, n), -1, np.int32)  # per witness slot the call and the voter that decided it (what the library records)
    dec_by = np.full((R, n), -1, np.int32)
    calls = []                               # (max_c, rounds, events divided) per call
    n_coin = n_weighted = n_by_stake = 0
    for call, (_, divided) in enumerate(g["batches"]):
        reg = (wit >= 0) & (wit < divided)   # the witnesses this call knows
        max_c = 0
        while max_c in consensus:
            max_c += 1
        max_r = int(np.nonzero(reg.any(axis=1))[0].max()) if reg.any() else -1
        calls.append((max_c, max_r + 1, int(divided)))
        done = set()
        for r_ in range(max_c + 1, max_r + 1):
            for mv in np.argsort(np.where(reg[r_], wit[r_], np.iinfo(np.int32).max), kind="stable"):
                if not reg[r_, mv]:
                    break
                y = int(wit[r_, mv])
                for r in range(max_c, r_):
                    if r in consensus:
                        continue
                    und = reg[r] & ~famous[r]
                    if not und.any():
                        continue
                    d = r_ - r
                    el = elections.get(r)
                    if el is None:
                        el = elections[r] = Election(g, S, r, coin_period)
                    V, strong, coined = el.level(d)
                    stored = und
                    if d > 1:
                        n_by_stake += int((und & el.by_stake[d][mv]).sum())
                    if d > 1 and d % coin_period != 0:
                        decided = und & strong[mv]
                        if decided.any():
                            famous[r] |= decided
                            dec_call[r, decided] = call
                            dec_by[r, decided] = y
                            done.add(r)
                        stored = und & ~strong[mv]
                    if stored.any():
                        row = rows.setdefault((y, r), [np.zeros(n, bool), np.zeros(n, bool)])
                        assert not (row[0] & stored & (row[1] != V[mv])).any(), "a vote stored twice keeps its value"
                        row[0] |= stored
                        row[1] |= stored & V[mv]
                        n_coin += int((stored & coined[mv]).sum())
                        if d > 1 and not unit:
                            n_weighted += int(stored.sum())
        mine = {r for r in done if (famous[r] | ~reg[r]).all()}
        assert mine == {int(r) for r in new_c[call]}, "call %d: new_c %s, recorded %s" % (call, sorted(mine), list(new_c[call]))
        consensus |= mine
    keys = sorted(rows, key=lambda k: (int(rnd[k[0]]), k[0], k[1]))
    nwo = (n + 63) // 64
    ex = np.zeros((len(keys), nwo * 64), bool)
    va = np.zeros((len(keys), nwo * 64), bool)
    for i, k in enumerate(keys):
        ex[i, :n], va[i, :n] = rows[k]
    return {"row_voter": np.array([k[0] for k in keys], np.int32), "row_cand_round": np.array([k[1] for k in keys], np.int32),
            "exists": pack_words(ex), "value": pack_words(va), "n_entries": int(ex.sum()), "n_coin": n_coin, "n_weighted": n_weighted,
            "n_by_stake": n_by_stake,
            "dec_call": dec_call, "dec_by": dec_by, "calls": calls, "S": S,
            "cons_call": np.array([next((i for i, nc in enumerate(new_c) if r in set(int(x) for x in nc)), -1) for r in range(R)], np.int32)}


def pack_words(bits):
    """bool [rows][64 nwo] -> uint64 [rows][nwo], bit i of word j = column 64 j + i"""
    rows, cols = bits.shape
    b = np.packbits(bits.reshape(rows, cols // 64, 64), axis=2, bitorder="little")   # [rows][nwo][8] bytes
    return np.ascontiguousarray(b).view("<u8").reshape(rows, cols // 64)


def unpack_words(words, n):
    """uint64 [rows][nwo] -> bool [rows][n]"""
    rows = words.shape[0]
    b = np.ascontiguousarray(words.astype("<u8")).view(np.uint8).reshape(rows, words.shape[1] * 8)
    return np.unpackbits(b, axis=1, bitorder="little")[:, :n].astype(bool)


def triples(row_voter, row_cand_round, exists, value, witnesses):
    """The table expanded to int64 [K, 3] rows (y, x, v): the layout of the goldens' `votes`."""
    n = witnesses.shape[1]
    ex, va = unpack_words(exists, n), unpack_words(value, n)
    i, mc = np.nonzero(ex)
    out = np.empty((len(i), 3), np.int64)
    out[:, 0] = row_voter[i]
    out[:, 1] = witnesses[row_cand_round[i], mc]
    out[:, 2] = va[i, mc]
    return out
