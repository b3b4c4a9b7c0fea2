"""ctypes binding of the C-ABI (include/swirld_hip.h).  The shared library is built
in-tree by `__graft_entry__.build()` / `py-swirld_amd/build.py`; there is NO fallback: if
the library is missing, or no GPU is present when a context is created, this fails
loudly."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libswirld_hip.so")

SW_OK = 0
ERRNO_NAMES = {-5: "SW_EIO", -12: "SW_ENOMEM", -19: "SW_ENODEV", -22: "SW_EINVAL",
               -34: "SW_ERANGE", -75: "SW_EOVERFLOW", -95: "SW_ENOTSUP"}


class SwirldHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERRNO_NAMES.get(code, "error"), code, msg))
        self.code = code


class Counters(C.Structure):
    _fields_ = [(k, C.c_int64) for k in (
        "events_divided", "rounds", "tally_evals", "round_iterations", "voter_evals",
        "majority_evals", "levels", "kernel_launches", "far_hops", "band_events", "coin_votes", "coin_flips",
        "chunk_sweeps", "chunk_provisional", "chunk_repaired", "chunk_resweeps", "finalize_from_rows", "order_rounds_host_sorted",
        "gated_calls", "gated_idle_iterations")]


# sw_gossip_turn's flags and stages (include/swirld_hip.h)
SW_TURN_VALIDATE, SW_TURN_DATA, SW_TURN_TRUNKS, SW_TURN_NO_CONSENSUS = 1, 2, 4, 8
SW_TURN_STAGE_NONE, SW_TURN_STAGE_PULLED, SW_TURN_STAGE_CREATED, SW_TURN_STAGE_DIVIDED, SW_TURN_STAGE_FAME, SW_TURN_STAGE_ORDERED = range(6)


class TurnResult(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_sent", "n_valid", "n_stored", "new_head", "n_new_rounds", "n_ordered", "stage")]


class Timings(C.Structure):
    _fields_ = [("can_see_ms", C.c_float), ("rounds_ms", C.c_float), ("tally_ms", C.c_float),
                ("tally_launches", C.c_int32), ("finalize_ms", C.c_float), ("fame_ms", C.c_float),
                ("total_ms", C.c_float), ("cansee_kernel_ms", C.c_float), ("cansee_launches", C.c_int32),
                ("resolve_ms", C.c_float), ("resolve_launches", C.c_int32), ("elections_ms", C.c_float)]


# name -> (restype, argtypes): every symbol include/swirld_hip.h declares
_P = C.c_void_p
SIGNATURES = {
    "sw_version": (C.c_int, []),
    "sw_create": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.POINTER(_P)]),
    "sw_destroy": (C.c_int, [_P]),
    "sw_last_error": (C.c_char_p, [_P]),
    "sw_reserve": (C.c_int, [_P, C.c_int64]),
    "sw_append_events": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P]),
    "sw_num_events": (C.c_int64, [_P]),
    "sw_append_events_device": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "sw_get_ingest_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_set_event_ids": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "sw_get_event_ids": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "sw_lookup_event_ids": (C.c_int, [_P, C.c_int64, _P, _P]),
    "sw_ingest_payload_device": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_ingest_payload": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_get_payload_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    "sw_divide_rounds": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "sw_decide_fame": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "sw_decide_fame_partial": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_int, C.POINTER(C.c_int)]),
    "sw_commit_fame": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int, C.POINTER(C.c_int)]),
    "sw_row_stride": (C.c_int, [_P]),
    "sw_get_tally_impl": (C.c_int, [_P]),
    "sw_cansee_range": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "sw_split_link": (C.c_int, [_P, C.c_int]),
    "sw_split_unlink": (C.c_int, [_P]),
    "sw_cansee_repair": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "sw_export_rows": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P]),
    "sw_import_rows": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P]),
    "sw_get_range_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_find_order": (C.c_int, [_P, _P, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "sw_get_height": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "sw_get_round": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "sw_get_can_see": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "sw_max_round": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "sw_get_witnesses": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "sw_get_famous": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "sw_get_famous_events": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "sw_get_consensus": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "sw_get_sees_mask": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "sw_get_vote": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int8)]),
    "sw_export_votes_device": (C.c_int, [_P, C.c_int, C.c_int, C.c_int64, _P, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    "sw_export_votes": (C.c_int, [_P, C.c_int, C.c_int, C.c_int64, _P, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_get_votes_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    "sw_get_known_heights": (C.c_int, [_P, C.c_int64, _P]),
    "sw_sync_diff": (C.c_int, [_P, C.c_int64, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_get_chain_events": (C.c_int, [_P, C.c_int, C.c_int32, C.c_int32, _P]),
    "sw_get_known_heights_device": (C.c_int, [_P, C.c_int64, _P, _P]),
    "sw_export_payload_device": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_export_payload": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_sync_pull": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_get_export_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    "sw_get_round_received": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "sw_get_consensus_time": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "sw_export_ordered_device": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "sw_export_ordered": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, _P, _P, _P]),
    "sw_get_consensus_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_crypto_verify_batch": (C.c_int, [C.c_int, C.c_int64, _P, _P, _P, _P, _P]),
    "sw_crypto_hash_batch": (C.c_int, [C.c_int, C.c_int64, _P, _P, _P]),
    "sw_set_member_keys": (C.c_int, [_P, _P, C.POINTER(C.c_int32)]),
    "sw_get_member_keys": (C.c_int, [_P, _P, _P]),
    "sw_validate_payload_device": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, _P, _P, C.c_int64, _P, _P, _P, _P, _P]),
    "sw_validate_payload": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "sw_get_validate_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    "sw_set_event_class": (C.c_int, [_P, C.c_char_p, C.c_char_p]),
    "sw_get_event_class": (C.c_int, [_P, _P, _P]),
    "sw_pack_bound": (C.c_int, [_P, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_pack_events_device": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int64, _P, _P, C.c_int64, _P, _P]),
    "sw_pack_events": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int64, _P, _P, C.c_int64, _P,
                                 C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_sync_pull_validated": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_get_pack_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    "sw_set_event_data": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, C.c_int64, _P]),
    "sw_set_event_data_device": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, C.c_int64, _P, _P]),
    "sw_get_event_data": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_gather_event_data_device": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_gather_event_data": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_ingest_payload_data_device": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), _P, _P, C.c_int64, _P]),
    "sw_ingest_payload_data": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), _P, _P, C.c_int64, _P]),
    "sw_sync_pull_data": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_get_data_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    "sw_get_fork_trunks": (C.c_int, [_P, _P]),
    "sw_sync_walk": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, _P, C.POINTER(C.c_int64)]),
    "sw_export_walk_device": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_export_walk": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_sync_pull_walk": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int64)]),
    "sw_get_walk_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    # the wire bytes of a sync answer (csrc/wire.hip.h)
    "sw_pack_message_bound": (C.c_int, [_P, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    "sw_pack_message_device": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, C.c_int64, _P, _P]),
    "sw_pack_message": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "sw_unpack_message_device": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_unpack_message": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_export_message_device": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int, _P, C.c_int64, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_export_message": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_ingest_message_device": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_ingest_message": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_get_wire_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_set_signing_keys":(C.c_int, [_P, C.c_int64, _P, _P]),
    "sw_clear_signing_keys": (C.c_int, [_P]),
    "sw_get_signing_members": (C.c_int, [_P, _P]),
    "sw_sign_events_device": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P]),
    "sw_sign_events": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "sw_create_events_device": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, C.POINTER(C.c_int64), _P, _P]),
    "sw_create_events": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, _P, C.POINTER(C.c_int64), _P, _P]),
    "sw_get_sign_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    # one event signed by one wavefront, and the gossip turn around it (csrc/turn.hip.h)
    "sw_create_event": (C.c_int, [_P, C.c_int, C.c_int64, C.c_int64, C.c_double, _P, C.c_int64, C.POINTER(C.c_int64), _P, _P]),
    "sw_gossip_turn": (C.c_int, [_P, C.c_int, C.c_int64, _P, C.c_int64, C.c_double, _P, C.c_int64, C.c_int, _P, C.c_int, _P, C.c_size_t]),
    "sw_get_turn_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P,
                                    C.POINTER(C.c_double)]),
    "sw_num_ordered":(C.c_int, [_P, C.POINTER(C.c_int64)]),
    "sw_get_transactions": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "sw_get_counters": (C.c_int, [_P, C.POINTER(Counters)]),
    "sw_get_counters_sized": (C.c_int, [_P, _P, C.c_size_t]),
    "sw_set_profiling": (C.c_int, [_P, C.c_int]),
    "sw_get_timings": (C.c_int, [_P, C.POINTER(Timings)]),
    "sw_debug_clocks": (C.c_int, [_P, _P, C.c_int64]),
    "sw_debug_block_clocks": (C.c_int, [_P, _P, C.c_int64]),
    "sw_debug_live_resources": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_set_forks": (C.c_int, [_P, C.c_int]),
    "sw_get_exact": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "sw_get_witness_order": (C.c_int, [_P, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    # the history of the exact path (csrc/exact_history.hip.h)
    "sw_set_exact_history": (C.c_int, [_P, C.c_int]),
    "sw_get_exact_history": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sw_get_votes_by_event": (C.c_int, [_P, C.c_int64, _P, _P, _P]),
    "sw_export_vote_entries_device": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, _P, C.POINTER(C.c_int64), _P]),
    "sw_export_vote_entries": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_get_vote_store_stats": (C.c_int, [_P] + [C.POINTER(C.c_int64)] * 7),
    # batches of small hashgraphs (csrc/batch.hip.h)
    "sw_batch_bytes": (C.c_int64, [C.c_int64, C.c_int, C.c_int64, C.c_int64]),
    "sw_batch_create": (C.c_int, [C.c_int64, C.c_int, _P, C.c_int, C.c_int64, C.c_int64, C.c_int, C.POINTER(_P)]),
    "sw_batch_destroy": (C.c_int, [_P]),
    "sw_batch_last_error": (C.c_char_p, [_P]),
    "sw_batch_shape": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                 C.POINTER(C.c_int64)]),
    "sw_batch_append": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "sw_batch_step": (C.c_int, [_P, _P, C.POINTER(C.c_int64)]),
    "sw_batch_get_summary": (C.c_int, [_P, _P]),
    "sw_batch_get_height": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P]),
    "sw_batch_get_round": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P]),
    "sw_batch_get_can_see": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P]),
    "sw_batch_get_witnesses": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, _P]),
    "sw_batch_get_witness_order": (C.c_int, [_P, C.c_int64, C.c_int, _P, C.POINTER(C.c_int)]),
    "sw_batch_get_famous": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, _P]),
    "sw_batch_get_famous_events": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P]),
    "sw_batch_get_consensus": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, _P]),
    "sw_batch_get_new_rounds": (C.c_int, [_P, C.c_int64, _P, C.c_int, C.POINTER(C.c_int)]),
    "sw_batch_get_transactions": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P, _P, _P]),
    # ... their histories generated on the device (csrc/batch_synth.hip.h)
    "sw_synth_batch_begin": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "sw_synth_batch": (C.c_int, [_P, _P, C.POINTER(C.c_int64)]),
    "sw_synth_batch_stats": (C.c_int, [_P, _P]),
    "sw_get_batch_events": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P, _P, _P, _P, _P]),
    # ... and their results, the whole batch per call (csrc/batch_export.hip.h)
    "sw_export_batch_ordered": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_export_batch_ordered_device": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, C.POINTER(C.c_int64), _P]),
    "sw_export_batch_new_rounds": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.POINTER(C.c_int64)]),
    "sw_export_batch_new_rounds_device": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.POINTER(C.c_int64), _P]),
    "sw_export_batch_events": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_export_batch_events_device": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), _P]),
    "sw_export_batch_rounds": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_export_batch_rounds_device": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, C.POINTER(C.c_int64), _P]),
    "sw_export_batch_stats": (C.c_int, [_P, _P]),
    # ... and gossip networks of consecutive hashgraphs (csrc/batch_network.hip.h)
    "sw_network_batch_begin": (C.c_int, [_P, _P, _P, _P, _P]),
    "sw_network_batch_turns": (C.c_int, [_P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sw_network_batch_run": (C.c_int, [_P, _P, C.POINTER(C.c_int64)]),
    "sw_network_batch_get": (C.c_int, [_P, _P]),
    "sw_network_batch_heads": (C.c_int, [_P, _P]),
    "sw_network_batch_stats": (C.c_int, [_P, _P]),
    "sw_get_network_event_numbers": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P]),
    "sw_export_network_event_numbers": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, C.POINTER(C.c_int64)]),
    "sw_export_network_event_numbers_device": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, C.POINTER(C.c_int64), _P]),
    "sw_synth_schedule": (C.c_int, [C.c_int, C.c_uint64, C.c_int64, C.c_int64, _P, _P]),
    "sw_set_window": (C.c_int, [_P, C.c_int, C.c_int]),
    "sw_get_window": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sw_set_window_lapse": (C.c_int, [_P, C.c_int64]),
    "sw_rewind": (C.c_int, [_P]),
    "sw_reset": (C.c_int, [_P]),
    "sw_synchronize": (C.c_int, [_P]),
    "sw_synth_hashgraph": (C.c_int, [C.c_int, C.c_int64, C.c_uint64, C.c_int, C.c_double,
                                     C.c_double, _P, _P, _P, _P, _P]),
}

_lib = None


def load():
    """Load libswirld_hip.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: the HIP extension has not been built (run "
                "`python -c 'import __graft_entry__ as g; g.build()'` or "
                "`python py-swirld_amd/build.py`).  There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)  # AttributeError if the symbol is not exported
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def hip_runtime_paths():
    """The HIP runtime libraries mapped into this process (paths of libamdhip64*).  PyTorch wheels carry their own copy with
    the SONAME of the system one: loaded FIRST, it also serves this library (one runtime, stream handles and events can be
    shared); loaded AFTER this library it becomes a SECOND runtime — its streams mean nothing to the C-ABI, and it may not even
    find the GPU once a windowed table has reserved its address range.  Import torch before this package when both are used."""
    paths = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    paths.add(os.path.realpath(line.split()[-1]))
    except OSError:
        pass
    return sorted(paths)


def require_single_hip_runtime(what):
    p = hip_runtime_paths()
    if len(p) > 1:
        raise RuntimeError("%s: two HIP runtimes are loaded in this process (%s) — torch was imported after py-swirld_amd; "
                           "import torch first, so that both use one runtime and stream handles can cross the C-ABI" % (what, ", ".join(p)))

