"""CPU: the tiled model of the device ingest (tests/model_ingest.py = csrc/ingest.hip.h step by step) against the
plain sequential loop and the oracle's heights, on generator streams of all four modes; every defect the C-ABI
names, injected at tile and wave boundaries; the rule that settles the verdict."""
import numpy as np
import pytest

import model_ingest as M

MODES = [(0, 0.0, 0.0), (1, 0.05, 0.0), (2, 0.25, 0.05), (3, 0.5, 0.0)]
SHAPES = [(16, 2, 4, 8), (32, 4, 8, 5), (8, 1, 8, 64)]   # tile, waves, wave, heights tile


def _same(a, b):
    for f in ("cr", "sp", "op", "seq", "ht", "nev", "head", "first"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


@pytest.mark.parametrize("mode,p0,p1", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_valid_streams_equal_the_sequential_loop_and_the_oracle(pkg, mode, p0, p1, shape):
    from oracle.oracle import Oracle
    n, N = 12, 700
    cr, sp, op, _, _ = pkg.synth_hashgraph(n, N, 11 + mode, mode, p0, p1)
    o = Oracle(n)
    o.append_events(cr, sp, op)
    tile, waves, wave, ht_tile = shape
    for cuts in ([0, N], [0, 233, 240, 513, N]):   # (cuts inside tiles and waves)
        a, b = M.State(n), M.State(n)
        for x, y in zip(cuts[:-1], cuts[1:]):
            va, a = M.ingest(a, cr[x:y], sp[x:y], op[x:y], tile, waves, wave, ht_tile)
            vb, b = M.sequential(b, cr[x:y], sp[x:y], op[x:y])
            assert va is None and vb is None
            _same(a, b)
        assert np.array_equal(a.ht, o.height)
        # chain positions are what the chain pool is scattered by: every member's events in index order
        for m in range(n):
            ev = np.nonzero(cr == m)[0]
            assert np.array_equal(a.seq[ev], np.arange(len(ev)))
            assert a.head[m] == ev[-1] and a.first[m] == ev[0] and a.nev[m] == len(ev)


def _defect(kind, cr, sp, op, k, N, n):
    cr, sp, op = cr.copy(), sp.copy(), op.copy()
    if kind == "creator_n":
        cr[k] = n
    elif kind == "creator_neg":
        cr[k] = -1
    elif kind == "one_parent":
        op[k] = -1
    elif kind == "own_index":
        sp[k] = k
    elif kind == "beyond_batch":
        op[k] = N + 5
    elif kind == "self_by_other":
        sp[k] = op[k]
    elif kind == "other_by_same":
        op[k] = sp[k]
    elif kind == "fork":
        sp[k] = sp[sp[k]]
    elif kind == "second_root":
        sp[k] = op[k] = -1
    return cr, sp, op


CODES = {"creator_n": M.V_CREATOR, "creator_neg": M.V_CREATOR, "one_parent": M.V_ARITY, "own_index": M.V_ORDER,
         "beyond_batch": M.V_ORDER, "self_by_other": M.V_SELF, "other_by_same": M.V_OTHER, "fork": M.V_FORK,
         "second_root": M.V_FORK}


@pytest.mark.parametrize("kind", sorted(CODES))
def test_every_defect_at_tile_and_wave_boundaries(pkg, kind):
    n, N = 6, 200
    cr, sp, op, _, _ = pkg.synth_hashgraph(n, N, 5)
    tile, waves, wave, ht_tile = 32, 2, 8, 8
    # last lane of a wave step, first of the next, last event of a wave's share, first of a tile, last of the batch
    for first_cut in (0, 50):   # as the first batch, and behind a committed one
        for pos in (39, 40, 47, 48, 63, 64, 65, 127, 128, N - first_cut - 1):
            k = first_cut + pos
            if kind == "fork" and sp[sp[k]] < 0:
                continue
            c2, s2, o2 = _defect(kind, cr, sp, op, k, N, n)
            st = M.State(n)
            if first_cut:
                _, st = M.ingest(st, cr[:first_cut], sp[:first_cut], op[:first_cut], tile, waves, wave, ht_tile)
            v, out = M.ingest(st, c2[first_cut:], s2[first_cut:], o2[first_cut:], tile, waves, wave, ht_tile)
            assert v == (k, CODES[kind]) and out is None, (kind, k, first_cut, v)
            assert M.sequential(st, c2[first_cut:], s2[first_cut:], o2[first_cut:])[0] == v


def test_lowest_event_wins_and_the_first_failing_check_of_it(pkg):
    n, N = 6, 200
    cr, sp, op, _, _ = pkg.synth_hashgraph(n, N, 6)
    kinds = sorted(CODES)
    rng = np.random.default_rng(3)
    for _ in range(60):
        ka, kb = (kinds[i] for i in rng.integers(0, len(kinds), 2))
        a, b = sorted(int(x) for x in rng.choice(np.arange(n + 8, N), 2, replace=False))
        if sp[sp[a]] < 0 or sp[sp[b]] < 0:
            continue
        c2, s2, o2 = _defect(ka, cr, sp, op, a, N, n)
        c2, s2, o2 = _defect(kb, c2, s2, o2, b, N, n)
        v, _ = M.ingest(M.State(n), c2, s2, o2, 32, 2, 8, 8)
        assert v == M.sequential(M.State(n), c2, s2, o2)[0]
        assert v[0] == a, (ka, a, kb, b, v)   # the later defect, and whatever the earlier one made later events look like, loses
    # several defects of ONE event: the order of the checks
    k = 100
    c2, s2, o2 = _defect("creator_n", cr, sp, op, k, N, n)
    c2, s2, o2 = _defect("one_parent", c2, s2, o2, k, N, n)
    assert M.ingest(M.State(n), c2, s2, o2)[0] == (k, M.V_CREATOR)
    c2, s2, o2 = _defect("one_parent", cr, sp, op, k, N, n)
    s2[k] = N + 1
    assert M.ingest(M.State(n), c2, s2, o2)[0] == (k, M.V_ARITY)
    c2, s2, o2 = cr.copy(), sp.copy(), op.copy()
    s2[k], o2[k] = op[k], op[k]          # self-parent by another member; other-parent then by that member, not the creator
    assert M.ingest(M.State(n), c2, s2, o2)[0] == (k, M.V_SELF)
    c2, s2, o2 = cr.copy(), sp.copy(), op.copy()
    s2[k], o2[k] = sp[sp[k]], sp[k]      # a fork whose other-parent is by the same member: the defect comes first
    assert M.ingest(M.State(n), c2, s2, o2)[0] == (k, M.V_OTHER)


def test_a_clamped_event_changes_later_verdict_words_only(pkg):
    """An event that fails a local check is left out of the ranks: the link checks may then call later events of its
    creator forks, but every such word lies above the clamped event's own — the minimum is unchanged."""
    n, N = 6, 200
    cr, sp, op, _, _ = pkg.synth_hashgraph(n, N, 7)
    for k in (31, 32, 33, 90):
        c2, s2, o2 = _defect("own_index", cr, sp, op, k, N, n)
        st = M.State(n)
        key, words = M.local_checks(c2.astype(np.int64), s2, o2, 0, n)
        assert key[k] == -1 and words == [(k << 8) | M.V_ORDER]
        hist, head, frst = M.tile_hist(key, 0, n, 32, st.head, st.first)
        base, _ = M.tile_scan(hist, st.nev)
        seq = M.tile_rank(key, base, n, 32, 2, 8)
        later = M.link_checks(st, key, s2, o2, seq, 0)
        assert later and all((w >> 8) > k for w in later)      # (its creator's next event does look like a fork)
        valid_seq = M.sequential(M.State(n), cr, sp, op)[1].seq
        assert np.array_equal(seq[:k], valid_seq[:k])          # ranks in front of it are untouched
        assert M.ingest(M.State(n), c2, s2, o2, 32, 2, 8, 8)[0] == (k, M.V_ORDER)


def test_heights_fixed_point_is_bounded_and_block_spans(pkg):
    n, N = 4, 400
    cr, sp, op, _, _ = pkg.synth_hashgraph(n, N, 9)
    ref = M.sequential(M.State(n), cr, sp, op)[1].ht
    for ht_tile in (1, 2, 7, 64, 1024):
        ht, worst, err = M.heights_tiled(np.zeros(0, np.int64), sp, op, 0, ht_tile)
        assert not err and np.array_equal(ht, ref)
        assert worst <= ht_tile                    # a chain inside a tile is at most the tile long
    # a batch behind committed events gathers their heights
    ht, _, err = M.heights_tiled(ref[:150], sp[150:], op[150:], 150, 16)
    assert not err and np.array_equal(ht, ref[150:])
    # an index that points INTO the tile at or behind the event never settles: the kernel's trip bound ends it
    s2 = sp.copy()
    s2[300] = 300
    assert M.heights_tiled(np.zeros(0, np.int64), s2, op, 0, 64)[2]
    spans = M.block_spans(ref[100:], 100, shift=6)
    for b, (lo, hi) in spans.items():
        seg = ref[max(100, b << 6):(b + 1) << 6]
        assert (lo, hi) == (seg.min(), seg.max())
