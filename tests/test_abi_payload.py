"""CPU: the entry points of the id index and of the payload ingest are exported and refuse a NULL context."""
import ctypes as C
import importlib

NEW = ("sw_set_event_ids", "sw_get_event_ids", "sw_lookup_event_ids", "sw_ingest_payload_device", "sw_ingest_payload",
       "sw_get_payload_stats")


def test_new_symbols_exported_and_bound(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    sig = importlib.import_module("py-swirld_amd._lib").SIGNATURES
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in sig, name
    assert lib.sw_version() == 7     # nothing existing changed signature


def test_null_context_is_einval(pkg):
    L = importlib.import_module("py-swirld_amd._lib").load()
    buf = (C.c_uint8 * 64)()
    out = (C.c_int32 * 2)()
    n = C.c_int64(5)
    assert L.sw_set_event_ids(None, 0, 1, buf) == -22
    assert L.sw_get_event_ids(None, 0, 1, buf) == -22
    assert L.sw_lookup_event_ids(None, 1, buf, out) == -22
    assert L.sw_ingest_payload(None, 1, buf, buf, buf, buf, out, None, None, None, out, C.byref(n)) == -22
    assert L.sw_ingest_payload_device(None, 1, buf, buf, buf, buf, out, None, None, None, None, out, C.byref(n)) == -22
    assert L.sw_get_payload_stats(None, None, None, None, None, None) == -22


def test_front_end_has_the_methods(pkg):
    for name in ("set_event_ids", "event_ids", "lookup_event_ids", "ingest_payload", "ingest_payload_device", "payload_stats"):
        assert callable(getattr(pkg.Hashgraph, name)), name
    assert pkg.Node.device_payload_threshold is None
