"""The gossip networks of a batch (csrc/batch_network.hip.h) as plain Python over per-view lists: the turn with the literal
BFS of swirld.py:154-159, the two generators, and — independent of it — the closed form: the schedule alone fixes the
network's DAG, and after node i's last turn view i is the set of ancestors of its head.  No GPU, no pytest."""
import numpy as np

M64 = (1 << 64) - 1


class Xoshiro:
    """csrc/synth.cpp's generator."""

    def __init__(self, seed):
        x = seed & M64
        self.s = []
        for _ in range(4):
            x = (x + 0x9E3779B97F4A7C15) & M64
            z = x
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
            self.s.append(z ^ (z >> 31))

    @staticmethod
    def _rotl(x, k):
        return ((x << k) | (x >> (64 - k))) & M64

    def next(self):
        s = self.s
        r = (self._rotl((s[1] * 5) & M64, 7) * 9) & M64
        t = (s[1] << 17) & M64
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t
        s[3] = self._rotl(s[3], 45)
        return r

    def below(self, n):
        return (self.next() * n) >> 64


def schedule_rng(seed):
    return Xoshiro((seed * 0x2545F4914F6CDD1D + 0x1234567 + 4) & M64)


def draw(rng, n):
    a = rng.below(n)
    b = rng.below(n - 1)
    return a, b + (b >= a)


def schedule(n, seed, first_turn, T):
    """What sw_synth_schedule writes."""
    rng = schedule_rng(seed)
    turns = [draw(rng, n) for _ in range(first_turn + T)][first_turn:]
    return np.array([a for a, _ in turns], np.int32), np.array([b for _, b in turns], np.int32)


def signature(rng):
    return np.frombuffer(b"".join(rng.next().to_bytes(8, "little") for _ in range(8)), np.uint8).copy()


class View:
    def __init__(self, n):
        self.n = n
        self.cr, self.sp, self.op, self.ht, self.t, self.sig, self.num = [], [], [], [], [], [], []
        self.idx = {}        # number -> local index
        self.can_see = []    # rows of n entries, -1 absent (swirld.py:203-205, 220: no round enters)
        self.head = -1
        self.steps = []      # (first, K) of the main-loop steps: the root's divide, then one per turn

    def store(self, cr, sp, op, t, sig, num):
        e = len(self.cr)
        ht = 0 if sp < 0 else max(self.ht[sp], self.ht[op]) + 1   # :117-120
        if sp < 0:
            row = [-1] * self.n
        else:
            def higher(a, b):
                return a >= 0 and (b < 0 or self.ht[a] >= self.ht[b])
            row = [a if higher(a, b) else b for a, b in zip(self.can_see[sp], self.can_see[op])]
        row[cr] = e
        self.cr.append(cr); self.sp.append(sp); self.op.append(op); self.ht.append(ht); self.t.append(t); self.sig.append(sig); self.num.append(num)
        self.idx[num] = e
        self.can_see.append(row)
        return e

    def arrays(self):
        return (np.array(self.cr, np.int32), np.array(self.sp, np.int32), np.array(self.op, np.int32), np.array(self.t, np.float64),
                np.array(self.sig, np.uint8).reshape(-1, 64))


class Network:
    def __init__(self, n, seed=0, root_t=None, root_sig=None):
        self.n, self.seed = n, seed
        self.sig_rng = Xoshiro(seed ^ 0xA5A5A5A5DEADBEEF)
        self.sched_rng = schedule_rng(seed)
        self.views = [View(n) for _ in range(n)]
        self.created = n
        self.turns = 0
        self.events = []   # per number: (creator, self-parent number, other-parent number), the network's DAG
        self.schedule = []
        for i, v in enumerate(self.views):
            g = signature(self.sig_rng)
            v.head = v.store(i, -1, -1, float(i) if root_t is None else float(root_t[i]), g if root_sig is None else np.asarray(root_sig[i], np.uint8), i)
            v.steps.append((0, 1))
            self.events.append((i, -1, -1))

    def answer(self, i, j):
        """swirld.py:154-159: the BFS in view j from its head, pruned by the heights node i reports (:125-126)."""
        vi, vj = self.views[i], self.views[j]
        known = [vi.ht[k] if k >= 0 else -1 for k in vi.can_see[vi.head]]
        seen, level = {vj.head}, [vj.head]
        while level:
            nxt = []
            for u in level:
                for p in (vj.sp[u], vj.op[u]):
                    if p < 0 or p in seen:
                        continue
                    if known[vj.cr[p]] < 0 or vj.ht[p] > known[vj.cr[p]]:
                        seen.add(p)
                        nxt.append(p)
            level = nxt
        return seen

    def turn(self, i, j, t=None, sig=None):
        assert i != j
        vi, vj = self.views[i], self.views[j]
        first = len(vi.cr)
        new = sorted(e for e in self.answer(i, j) if vj.num[e] not in vi.idx)   # :130, ascending local index of j
        for e in new:   # every parent resolves: held, or earlier in the list
            for p in (vj.sp[e], vj.op[e]):
                if p >= 0:
                    assert vj.num[p] in vi.idx or (p in new and new.index(p) < new.index(e)), "BROKEN"
        for e in new:   # :133-136
            sp = -1 if vj.sp[e] < 0 else vi.idx[vj.num[vj.sp[e]]]
            op = -1 if vj.op[e] < 0 else vi.idx[vj.num[vj.op[e]]]
            vi.store(vj.cr[e], sp, op, vj.t[e], vj.sig[e], vj.num[e])
        number = self.created
        g = signature(self.sig_rng)   # the stream advances whether or not a signature is given
        self.events.append((i, vi.num[vi.head], vj.num[vj.head]))
        vi.head = vi.store(i, vi.head, vi.idx[vj.num[vj.head]], float(number) if t is None else float(t), g if sig is None else np.asarray(sig, np.uint8), number)
        vi.steps.append((first, len(new) + 1))
        self.created += 1
        self.turns += 1
        self.schedule.append((i, j))
        return len(new)

    def run(self, T):
        for _ in range(T):
            self.turn(*draw(self.sched_rng, self.n))


def closed_form(n, sched):
    """The network's DAG from the schedule alone, and per node the numbers of the ancestors of its head."""
    events = [(i, -1, -1) for i in range(n)]
    head = list(range(n))
    anc = [{i} for i in range(n)]          # per number: its ancestors, itself included
    for i, j in sched:
        k = len(events)
        events.append((i, head[i], head[j]))
        anc.append(anc[head[i]] | anc[head[j]] | {k})
        head[i] = k
    return events, [anc[h] for h in head]


def oracle_of_view(n, mv, stake=None, coin_period=6):
    """The C oracle fed a model view's events under the view's step sizes: (oracle, transactions, failed step or None).
    The first step is the root's divide alone (swirld.py:75-80), every later one a main-loop step (:325-328)."""
    from oracle.oracle import Oracle, OracleError
    o = Oracle(n, stake, coin_period)
    cr, sp, op, t, sig = mv.arrays()
    tx = []
    for k, (first, K) in enumerate(mv.steps):
        o.append_events(cr[first:first + K], sp[first:first + K], op[first:first + K], t[first:first + K], sig[first:first + K])
        o.divide_rounds(first, K)
        if k == 0:
            continue
        try:
            tx += list(o.find_order(o.decide_fame()))
        except OracleError:
            return o, tx, k
    return o, tx, None


# ---- a network that stops: whale stakes (tests/batch_cases.py), a drawn schedule of 300 turns --------------------------------
def first_stop(n, stake, seed, T=300):
    """The earliest turn at which any puller's step raises, and who: what test() would have died at."""
    m = Network(n, seed)
    m.run(T)
    best = None
    for i, v in enumerate(m.views):
        _, _, failed = oracle_of_view(n, v, stake)
        if failed is not None:
            turn = [k for k, (a, _) in enumerate(m.schedule) if a == i][failed - 1]
            if best is None or turn < best[0]:
                best = (turn, i)
    return best


def find_stopping_seed(limit=2000):
    """(seed, (turn, puller)) of the first seed below `limit` whose network stops, or None."""
    from batch_cases import WHALE_N, whale_stake
    for seed in range(limit):
        hit = first_stop(WHALE_N, whale_stake(), seed)
        if hit is not None:
            return seed, hit
    return None


# what the search finds (tests/test_batch_network_host.py asserts it): seed 0 — node 4's pull in turn 184 raises swirld.py:305
STOPPING_NETWORK = (0, (184, 4))
