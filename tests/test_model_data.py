"""CPU: tests/model_data.py — the numpy statement of the data store, its gather, the ingest append and the ok-folding rule —
held against plain Python lists of bytes | None."""
import numpy as np

import model_data as md

LENS = [None, 0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 4095, 60000]


def datas(lens, seed):
    rng = np.random.default_rng(seed)
    return [None if n is None else rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]


def test_pack_and_unpack_are_inverse():
    d = datas(LENS + [0, None, 3], 1)
    data, off, none = md.pack(d)
    assert off[0] == 0 and off[-1] == len(data) == sum(len(x) for x in d if x is not None)
    assert none.tolist() == [x is None for x in d]
    assert md.unpack(data, off, none) == d
    assert md.unpack(*md.pack([])) == []


def test_store_set_get_gather_follow_the_lists():
    d = datas(LENS * 3, 2)
    st = md.Store()
    assert st.set(0, len(d), *md.pack(d[:10])) == 0
    assert st.set(10, len(d), *md.pack(d[10:])) == 0
    assert st.events == len(d) and st.as_list() == d
    assert md.unpack(*st.get(7, 20)) == d[7:27]
    assert st.get(7, 20)[1][0] == 0
    rng = np.random.default_rng(3)
    ev = rng.integers(0, len(d), 100)
    assert md.unpack(*st.gather(ev)) == [d[i] for i in ev]
    assert md.unpack(*st.gather(np.arange(len(d))[::-1])) == d[::-1]
    assert md.unpack(*st.gather([])) == []
    assert st.gather([0, len(d)]) == "SW_ERANGE" and st.gather([-1]) == "SW_ERANGE"


def test_store_refusals_store_nothing():
    d = datas([3, None, 5], 4)
    st = md.Store()
    assert st.set(1, 10, *md.pack(d)) == "SW_EINVAL"          # not at the number of events that have data
    assert st.set(0, 2, *md.pack(d)) == "SW_ERANGE"           # beyond the stored events
    data, off, none = md.pack(d)
    for bad in ([0, 3, 2, 8], [-1, 3, 3, 8], [0, 3, 3, 9]):
        assert st.set(0, 10, data, np.array(bad, np.int64), none) == "SW_EINVAL"
    long = np.zeros(md.MAX_DATA + 1, np.uint8)
    assert st.set(0, 10, long, np.array([0, md.MAX_DATA + 1], np.int64), None) == "SW_EINVAL"
    assert st.events == 0 and st.off == [0] and not st.data
    assert st.set(0, 10, None, None, None, K=4) == 0           # every event None
    assert st.as_list() == [None] * 4


def test_a_none_flag_wins_over_its_range():
    data, off, none = md.pack([b"abc", b"de"])
    st = md.Store()
    assert st.set(0, 2, data, off, np.array([1, 0], np.uint8)) == 0
    assert st.as_list() == [None, b"de"] and bytes(st.data) == b"de" and st.off == [0, 0, 2]


def test_fold_ok():
    off = np.array([0, 10, 5, 20, 20, 10 ** 12, 30, 31], np.int64)
    #            [0,10) ok; [10,5) decreasing; [5,20) ok; [20,20) ok; beyond; from beyond: decreasing; [30,31) beyond 30 bytes
    assert md.fold_ok(7, None, off, 30).tolist() == [1, 0, 1, 1, 0, 0, 0]
    assert md.fold_ok(7, [1, 1, 0, 2, 1, 1, 1], off, 31).tolist() == [1, 0, 0, 1, 0, 0, 1]
    assert md.fold_ok(3, None, None, 0).tolist() == [1, 1, 1]
    assert md.fold_sum(7, md.fold_ok(7, None, off, 30), off) == 10 + 15 + 0 and md.fold_sum(3, [1, 1, 1], None) == 0
    shared = np.array([0, 60000, 0, 60000, 0], np.int64)            # every second event accepted, all on ONE range
    assert md.fold_ok(4, None, shared, 60000).tolist() == [1, 0, 1, 0] and md.fold_sum(4, [1, 0, 1, 0], shared) == 120000 > 60000
    assert md.fold_ok(2, None, np.array([0, md.MAX_DATA, 2 * md.MAX_DATA + 1], np.int64), 10 ** 6).tolist() == [1, 0]


def test_ingest_append_is_in_dense_order():
    d = datas([4, None, 0, 7, 2, 9], 5)
    st = md.Store()
    st.set(0, 3, *md.pack([b"x", None, b"yz"]))
    #            payload position:  0   1   2   3  4  5       (3 events stored before; position 4 repeats position 0's id)
    index_out = np.array([5, -3, 3, 1, 5, 4], np.int32)
    st.ingest_append(index_out, 3, 3, *md.pack(d))
    assert st.as_list() == [b"x", None, b"yz", d[2], d[5], d[0]]
    assert md.slots(index_out, 3, 3).tolist() == [2, 5, 0]
