"""ctypes binding of libggrs_hip.so -- the C ABI declared in include/ggrs_hip.h.

The product path has NO CPU fallback: if the HIP extension is missing this module raises at
import time, and world creation raises when no gfx950 device is visible.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libggrs_hip.so")

GGRS_OK = 0
GGRS_E_INVALID = -1
GGRS_E_NO_SNAPSHOT = -2
GGRS_E_CAPACITY = -3
GGRS_E_HIP = -4
GGRS_E_NO_DEVICE = -5

GGRS_WORLD_DEFAULT = 0
GGRS_WORLD_UNFUSED = 2
GGRS_WORLD_NT_COPY = 4
GGRS_WORLD_NO_GROUPS = 8
GGRS_WORLD_LAYOUT_ONLY = 16

SYS_PARTICLES_UPDATE = 1
SYS_TTL_DESPAWN = 2
SYS_PARTICLES_SPAWN = 3
SYS_ADD_U32 = 4
SYS_SAT_SUB_DESPAWN = 5
SYS_BOX_MOVE = 6
SYS_CUSTOM = 7
SYS_SPAWN_CUSTOM = 8

INPUT_CONFIRMED, INPUT_PREDICTED, INPUT_DISCONNECTED = 0, 1, 2
MAX_INPUT_BYTES, MAX_PLAYERS = 16, 16
TIMELINE_FIELDS = 7

COMP_ROLLBACK, COMP_NO_ROLLBACK = 0, 1
DESPAWN_IMMEDIATE, DESPAWN_ROLLBACK = 0, 1

REQ_SAVE, REQ_LOAD, REQ_ADVANCE = 1, 2, 3

FANOUT_ID_BYTES = 128

KERNEL_SAVE, KERNEL_LOAD, KERNEL_ADVANCE, KERNEL_CHECKSUM, KERNEL_TICK, KERNEL_CLASSES = 0, 1, 2, 3, 4, 5


class WorldDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_depth", C.c_uint32), ("capacity", C.c_uint64),
                ("stream", C.c_void_p), ("arena", C.c_void_p), ("arena_bytes", C.c_uint64),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class SystemDesc(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("comp", C.c_uint32 * 4), ("word", C.c_uint32 * 4),
                ("iparam", C.c_int64 * 2), ("fparam", C.c_float * 4)]


CUSTOM_MAX_BINDINGS = 8


class CustomSystemDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("source", C.c_char_p), ("n_bindings", C.c_uint32),
                ("comp", C.c_uint32 * CUSTOM_MAX_BINDINGS), ("word", C.c_uint32 * CUSTOM_MAX_BINDINGS),
                ("iparam", C.c_int64 * 2), ("fparam", C.c_float * 4)]


PEER_MAX_BINDINGS = 8


class PeerBinding(C.Structure):
    _fields_ = [("comp", C.c_uint32), ("word", C.c_uint32)]


EFFECT_ADD, EFFECT_MIN_U, EFFECT_MAX_U, EFFECT_MIN_I, EFFECT_MAX_I, EFFECT_OR, EFFECT_AND, EFFECT_XOR = range(8)
EFFECT_MAX_BINDINGS = 8
EFFECT_MAX_COLUMNS = 8


class EffectBinding(C.Structure):
    _fields_ = [("comp", C.c_uint32), ("word", C.c_uint32), ("op", C.c_uint32)]


CMD_INSERT, CMD_REMOVE = 1, 2
COMMAND_MAX_BINDINGS = 4
COMMAND_MAX_WORDS = 8


class CommandBinding(C.Structure):
    _fields_ = [("comp", C.c_uint32), ("flags", C.c_uint32)]


SYS_RESOURCE = 9
RESOURCE_MAX, RESOURCE_MAX_BYTES, RESOURCE_MAX_BINDINGS = 8, 64, 8


class ResourceBinding(C.Structure):
    _fields_ = [("res", C.c_uint32), ("word", C.c_uint32)]


REDUCE_MAX_BINDINGS = 8


class ReduceBinding(C.Structure):
    _fields_ = [("res", C.c_uint32), ("word", C.c_uint32), ("op", C.c_uint32)]


REMOTE_INSERT, REMOTE_REMOVE, REMOTE_DESPAWN = 1, 2, 4
REMOTE_ENTITY = 0xFFFFFFFF
REMOTE_MAX_BINDINGS, REMOTE_MAX_COMPONENTS = 4, 8


class RemoteBinding(C.Structure):
    _fields_ = [("comp", C.c_uint32), ("flags", C.c_uint32)]


SUM_MAX_BINDINGS, SUM_MAX_WORDS = 4, 8


class SumBinding(C.Structure):
    _fields_ = [("res", C.c_uint32), ("word", C.c_uint32)]


VALUE_MAX_BINDINGS, VALUE_MAX_WORDS, VALUE_MAX_WORLD_BINDINGS = 4, 8, 16


class ValueBinding(C.Structure):
    _fields_ = [("comp", C.c_uint32), ("flags", C.c_uint32)]


class ResourceSystemDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("source", C.c_char_p), ("n_bindings", C.c_uint32),
                ("res", C.c_uint32 * RESOURCE_MAX_BINDINGS), ("word", C.c_uint32 * RESOURCE_MAX_BINDINGS),
                ("iparam", C.c_int64 * 2), ("fparam", C.c_float * 4)]


class SpawnSystemDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("source", C.c_char_p), ("bundle_mask", C.c_uint64), ("payload_stride", C.c_uint32), ("n_bindings", C.c_uint32),
                ("comp", C.c_uint32 * CUSTOM_MAX_BINDINGS), ("word", C.c_uint32 * CUSTOM_MAX_BINDINGS),
                ("iparam", C.c_int64 * 2), ("fparam", C.c_float * 4)]


class Request(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("frame", C.c_int32), ("dt_bits", C.c_uint32),
                ("n_inputs", C.c_uint32), ("inputs", C.POINTER(C.c_uint8)), ("status", C.POINTER(C.c_uint8)),
                ("spawn_count", C.c_uint64), ("spawn_vx", C.POINTER(C.c_float)),
                ("spawn_vy", C.POINTER(C.c_float)), ("spawn_payload", C.c_void_p), ("spawn_payload_bytes", C.c_uint64)]


class BranchSpawn(C.Structure):
    _fields_ = [("count", C.c_uint64), ("vx", C.c_void_p), ("vy", C.c_void_p), ("payload", C.c_void_p), ("payload_bytes", C.c_uint64)]


class BranchStep(C.Structure):
    _fields_ = [("prefix", C.POINTER(Request)), ("n_prefix", C.c_uint32), ("n_branches", C.c_uint32), ("n_frames", C.c_uint32), ("n_inputs", C.c_uint32),
                ("flags", C.c_uint32), ("n_spawn_table", C.c_uint32), ("inputs", C.c_void_p), ("status", C.c_void_p),
                ("spawn_table", C.POINTER(BranchSpawn)), ("spawn_sel", C.c_void_p)]


BRANCH_SAVE_LAST, BRANCH_RETAIN_NEWEST, BRANCH_RETAIN_ALL = 1, 2, 4
ADOPT_RECOMPUTE, ADOPT_BROADCAST = 0, 1

KERNEL_FORM_TILES, KERNEL_FORM_STEADY = 1, 3

DIFF_LIVE = -(1 << 31)            # GGRS_DIFF_LIVE: as a frame, the live world
DIFF_TRUST_VERSIONS = 1           # GGRS_DIFF_TRUST_VERSIONS


class DiffEntry(C.Structure):
    _fields_ = [("slot", C.c_uint64), ("alive_a", C.c_uint32), ("alive_b", C.c_uint32), ("presence_diff", C.c_uint64), ("column_diff", C.c_uint64),
                ("first_comp", C.c_uint32), ("first_word", C.c_uint32), ("first_a", C.c_uint64), ("first_b", C.c_uint64)]


class DiffReport(C.Structure):
    _fields_ = [("len_a", C.c_uint64), ("len_b", C.c_uint64), ("n_entities", C.c_uint64), ("n_alive", C.c_uint64),
                ("n_presence", C.c_uint64 * 64), ("n_value", C.c_uint64 * 64), ("resource_diff", C.c_uint64), ("n_entries", C.c_uint32)]


PART_COMPONENT, PART_ENTITY, PART_RESOURCE = 0, 1, 2      # GGRS_PART_*: the kind of a ggrs_checksum_part


class ChecksumPart(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("id", C.c_uint32), ("value", C.c_uint64), ("n_hashed", C.c_uint64)]


class PartsReport(C.Structure):
    _fields_ = [("len", C.c_uint64), ("active", C.c_uint64), ("checksum_lo", C.c_uint64), ("checksum_hi", C.c_uint64), ("n_parts", C.c_uint32)]


MAX_PARTS = 32 + 1 + 8                                    # GGRS_MAX_COMPONENTS components, the entities, GGRS_RESOURCE_MAX resources

QUERY_MAX_WORDS = 32                                      # GGRS_QUERY_MAX_WORDS
QUERY_SLOTS = 1                                           # GGRS_QUERY_SLOTS: also write each row's slot (u32)


class QueryWord(C.Structure):
    _fields_ = [("comp", C.c_uint32), ("word", C.c_uint32)]


class QueryDesc(C.Structure):
    _fields_ = [("with_mask", C.c_uint64), ("without_mask", C.c_uint64), ("n_words", C.c_uint32), ("flags", C.c_uint32), ("words", QueryWord * QUERY_MAX_WORDS)]


class QueryLayout(C.Structure):
    _fields_ = [("total_bytes", C.c_uint64), ("slots_off", C.c_uint64), ("col_off", C.c_uint64 * QUERY_MAX_WORDS), ("word_bytes", C.c_uint32 * QUERY_MAX_WORDS)]


class QueryReport(C.Structure):
    _fields_ = [("len", C.c_uint64), ("n_matched", C.c_uint64), ("n_rows", C.c_uint64)]


SCATTER_WRITE, SCATTER_INSERT, SCATTER_REMOVE, SCATTER_DESPAWN = 0, 1, 2, 3      # GGRS_SCATTER_*
SCATTER_OPS = {"write": SCATTER_WRITE, "insert": SCATTER_INSERT, "remove": SCATTER_REMOVE, "despawn": SCATTER_DESPAWN}


class ScatterDesc(C.Structure):
    _fields_ = [("op", C.c_uint32), ("flags", C.c_uint32), ("comp_mask", C.c_uint64), ("n_words", C.c_uint32), ("pad", C.c_uint32), ("words", QueryWord * QUERY_MAX_WORDS)]


class ScatterReport(C.Structure):
    _fields_ = [("len", C.c_uint64), ("n_rows", C.c_uint64), ("n_applied", C.c_uint64), ("n_dead", C.c_uint64), ("n_absent", C.c_uint64), ("first_bad_row", C.c_uint64)]


DELTA_CHANGED, DELTA_ADDED, DELTA_REMOVED, DELTA_DESPAWNED = 0, 1, 2, 3         # GGRS_DELTA_*
DELTA_KINDS = {"changed": DELTA_CHANGED, "added": DELTA_ADDED, "removed": DELTA_REMOVED, "despawned": DELTA_DESPAWNED}
DELTA_TRUST_VERSIONS = 1                                                        # GGRS_DELTA_TRUST_VERSIONS


class DeltaDesc(C.Structure):
    _fields_ = [("q", QueryDesc), ("changed_mask", C.c_uint64), ("kind", C.c_uint32), ("flags", C.c_uint32)]


class DeltaReport(C.Structure):
    _fields_ = [("len_new", C.c_uint64), ("len_old", C.c_uint64), ("n_matched", C.c_uint64), ("n_rows", C.c_uint64), ("n_beyond_old_len", C.c_uint64)]


SORT_MAX_KEYS = 4                                                               # GGRS_SORT_MAX_KEYS
SORT_U, SORT_I, SORT_F, SORT_DESC = 0, 1, 2, 0x100                              # GGRS_SORT_*
SORT_KINDS = {"u": SORT_U, "i": SORT_I, "f": SORT_F}


class SortKey(C.Structure):
    _fields_ = [("comp", C.c_uint32), ("word", C.c_uint32), ("kind", C.c_uint32)]


class SortDesc(C.Structure):
    _fields_ = [("keys", SortKey * SORT_MAX_KEYS), ("n_keys", C.c_uint32), ("flags", C.c_uint32)]


class PeerIndexDesc(C.Structure):
    _fields_ = [("comp", C.c_uint32), ("word", C.c_uint32), ("n_buckets", C.c_uint32), ("flags", C.c_uint32)]


PEER_INDEX_MAX_BUCKETS = 65535                                 # GGRS_PEER_INDEX_MAX_BUCKETS

# every symbol include/ggrs_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SIGNATURES = {
    "ggrs_hip_abi_version": (C.c_int, []),
    "ggrs_hip_device_count": (C.c_int, []),
    "ggrs_hip_world_create": (C.c_int, [C.c_int, C.c_uint64, C.c_uint32, C.POINTER(_P)]),
    "ggrs_hip_world_create_ex": (C.c_int, [C.POINTER(WorldDesc), C.POINTER(_P)]),
    "ggrs_hip_arena_bytes": (C.c_uint64, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]),
    "ggrs_hip_world_destroy": (None, [_P]),
    "ggrs_hip_last_error": (C.c_char_p, [_P]),
    "ggrs_hip_register_component": (C.c_int, [_P, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ggrs_hip_register_component_ex": (C.c_int, [_P, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ggrs_hip_set_component_default": (C.c_int, [_P, C.c_uint32, _P]),
    "ggrs_hip_checksum_component": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32]),
    "ggrs_hip_checksum_component_custom": (C.c_int, [_P, C.c_uint32, C.c_char_p]),
    "ggrs_hip_add_system": (C.c_int, [_P, C.POINTER(SystemDesc)]),
    "ggrs_hip_add_custom_system": (C.c_int, [_P, C.POINTER(CustomSystemDesc)]),
    "ggrs_hip_add_custom_system_peers": (C.c_int, [_P, C.POINTER(CustomSystemDesc), C.POINTER(PeerBinding), C.c_uint32]),
    "ggrs_hip_register_peer_index": (C.c_int, [_P, C.POINTER(PeerIndexDesc)]),
    "ggrs_hip_peer_index_read": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "ggrs_hip_add_custom_system_effects": (C.c_int, [_P, C.POINTER(CustomSystemDesc), C.POINTER(PeerBinding), C.c_uint32, C.POINTER(EffectBinding), C.c_uint32]),
    "ggrs_hip_add_custom_system_commands": (C.c_int, [_P, C.POINTER(CustomSystemDesc), C.POINTER(PeerBinding), C.c_uint32, C.POINTER(EffectBinding), C.c_uint32,
                                                      C.POINTER(CommandBinding), C.c_uint32]),
    "ggrs_hip_add_custom_system_resources": (C.c_int, [_P, C.POINTER(CustomSystemDesc), C.POINTER(PeerBinding), C.c_uint32, C.POINTER(EffectBinding), C.c_uint32,
                                                       C.POINTER(CommandBinding), C.c_uint32, C.POINTER(ResourceBinding), C.c_uint32]),
    "ggrs_hip_add_custom_system_reduces": (C.c_int, [_P, C.POINTER(CustomSystemDesc), C.POINTER(PeerBinding), C.c_uint32, C.POINTER(EffectBinding), C.c_uint32,
                                                     C.POINTER(CommandBinding), C.c_uint32, C.POINTER(ResourceBinding), C.c_uint32, C.POINTER(ReduceBinding), C.c_uint32]),
    "ggrs_hip_add_custom_system_remote": (C.c_int, [_P, C.POINTER(CustomSystemDesc), C.POINTER(PeerBinding), C.c_uint32, C.POINTER(EffectBinding), C.c_uint32,
                                                    C.POINTER(CommandBinding), C.c_uint32, C.POINTER(ResourceBinding), C.c_uint32, C.POINTER(ReduceBinding), C.c_uint32,
                                                    C.POINTER(RemoteBinding), C.c_uint32]),
    "ggrs_hip_add_custom_system_sums": (C.c_int, [_P, C.POINTER(CustomSystemDesc), C.POINTER(PeerBinding), C.c_uint32, C.POINTER(EffectBinding), C.c_uint32,
                                                  C.POINTER(CommandBinding), C.c_uint32, C.POINTER(ResourceBinding), C.c_uint32, C.POINTER(ReduceBinding), C.c_uint32,
                                                  C.POINTER(RemoteBinding), C.c_uint32, C.POINTER(SumBinding), C.c_uint32]),
    "ggrs_hip_add_custom_system_values": (C.c_int, [_P, C.POINTER(CustomSystemDesc), C.POINTER(PeerBinding), C.c_uint32, C.POINTER(EffectBinding), C.c_uint32,
                                                    C.POINTER(CommandBinding), C.c_uint32, C.POINTER(ResourceBinding), C.c_uint32, C.POINTER(ReduceBinding), C.c_uint32,
                                                    C.POINTER(RemoteBinding), C.c_uint32, C.POINTER(SumBinding), C.c_uint32, C.POINTER(ValueBinding), C.c_uint32]),
    "ggrs_hip_register_resource": (C.c_int, [_P, C.c_char_p, C.c_uint32, C.c_uint32, _P, C.POINTER(C.c_uint32)]),
    "ggrs_hip_checksum_resource": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32]),
    "ggrs_hip_add_resource_system": (C.c_int, [_P, C.POINTER(ResourceSystemDesc)]),
    "ggrs_hip_resource_read": (C.c_int, [_P, C.c_uint32, _P]),
    "ggrs_hip_resource_write": (C.c_int, [_P, C.c_uint32, _P]),
    "ggrs_hip_register_component_strategy": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p]),
    "ggrs_hip_set_input_layout": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "ggrs_hip_add_spawn_system": (C.c_int, [_P, C.POINTER(SpawnSystemDesc)]),
    "ggrs_hip_generated_kernel_source": (C.c_int, [_P, C.c_uint32, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_int]),
    "ggrs_hip_aot_object_name": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint64]),
    "ggrs_hip_host_timeline": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "ggrs_hip_set_frame_rate": (C.c_int, [_P, C.c_uint64]),
    "ggrs_hip_spawn": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "ggrs_hip_despawn": (C.c_int, [_P, C.c_uint64]),
    "ggrs_hip_despawn_rollback": (C.c_int, [_P, C.c_uint64]),
    "ggrs_hip_download_disabled": (C.c_int, [_P, _P, C.c_uint64]),
    "ggrs_hip_download_despawned_frames": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P]),
    "ggrs_hip_insert_component": (C.c_int, [_P, C.c_uint32, C.c_uint64, _P]),
    "ggrs_hip_remove_component": (C.c_int, [_P, C.c_uint32, C.c_uint64]),
    "ggrs_hip_upload_word": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _P]),
    "ggrs_hip_download_word": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _P]),
    "ggrs_hip_download_alive": (C.c_int, [_P, _P, C.c_uint64]),
    "ggrs_hip_download_present": (C.c_int, [_P, C.c_uint32, _P, C.c_uint64]),
    "ggrs_hip_column_device_ptr": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "ggrs_hip_len": (C.c_uint64, [_P]),
    "ggrs_hip_active_count": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "ggrs_hip_frame": (C.c_int32, [_P]),
    "ggrs_hip_set_frame": (C.c_int, [_P, C.c_int32]),
    "ggrs_hip_set_depth": (C.c_int, [_P, C.c_uint32]),
    "ggrs_hip_set_confirmed": (C.c_int, [_P, C.c_int, C.c_int32]),
    "ggrs_hip_has_snapshot": (C.c_int, [_P, C.c_int32]),
    "ggrs_hip_snapshot_count": (C.c_uint64, [_P]),
    "ggrs_hip_save": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "ggrs_hip_load": (C.c_int, [_P, C.c_int32]),
    "ggrs_hip_advance": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint64,
                                   C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ggrs_hip_handle_requests": (C.c_int, [_P, C.POINTER(Request), C.c_uint32, C.POINTER(C.c_uint64)]),
    "ggrs_hip_enqueue_requests": (C.c_int, [_P, C.POINTER(Request), C.c_uint32, C.POINTER(C.c_uint32)]),
    "ggrs_hip_collect_checksums": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32)]),
    "ggrs_hip_pending_batches": (C.c_uint32, [_P]),
    "ggrs_hip_set_synctest_check_distance": (C.c_int, [_P, C.c_int32]),
    "ggrs_hip_synchronize": (C.c_int, [_P]),
    "ggrs_hip_state_bytes": (C.c_uint64, [_P]),
    "ggrs_hip_live_state_ptr": (C.c_int, [_P, C.POINTER(_P)]),
    "ggrs_hip_adopt_live_state": (C.c_int, [_P]),
    "ggrs_hip_snapshot_copy": (C.c_int, [_P, C.c_int32, _P]),
    "ggrs_hip_diff_frames": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(DiffReport), C.POINTER(DiffEntry), C.c_uint32]),
    "ggrs_hip_diff_block": (C.c_int, [_P, C.c_int32, _P, C.c_uint32, C.POINTER(DiffReport), C.POINTER(DiffEntry), C.c_uint32]),
    "ggrs_hip_checksum_parts": (C.c_int, [_P, C.c_int32, C.POINTER(PartsReport), C.POINTER(ChecksumPart), C.c_uint32]),
    "ggrs_hip_checksum_parts_block": (C.c_int, [_P, _P, C.POINTER(PartsReport), C.POINTER(ChecksumPart), C.c_uint32]),
    "ggrs_hip_query_layout": (C.c_int, [_P, C.POINTER(QueryDesc), C.c_uint64, C.POINTER(QueryLayout)]),
    "ggrs_hip_query": (C.c_int, [_P, C.c_int32, C.POINTER(QueryDesc), _P, C.c_uint64, C.POINTER(QueryReport)]),
    "ggrs_hip_query_block": (C.c_int, [_P, _P, C.POINTER(QueryDesc), _P, C.c_uint64, C.POINTER(QueryReport)]),
    "ggrs_hip_query_sorted": (C.c_int, [_P, C.c_int32, C.POINTER(QueryDesc), C.POINTER(SortDesc), _P, C.c_uint64, C.POINTER(QueryReport)]),
    "ggrs_hip_query_sorted_block": (C.c_int, [_P, _P, C.POINTER(QueryDesc), C.POINTER(SortDesc), _P, C.c_uint64, C.POINTER(QueryReport)]),
    "ggrs_hip_scatter": (C.c_int, [_P, C.POINTER(ScatterDesc), _P, C.c_uint64, C.c_uint64, C.POINTER(ScatterReport)]),
    "ggrs_hip_delta_frames": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(DeltaDesc), _P, C.c_uint64, C.POINTER(DeltaReport)]),
    "ggrs_hip_delta_block": (C.c_int, [_P, C.c_int32, _P, C.POINTER(DeltaDesc), _P, C.c_uint64, C.POINTER(DeltaReport)]),
    "ggrs_hip_fanout_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "ggrs_hip_fanout_init": (C.c_int, [_P, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.POINTER(_P)]),
    "ggrs_hip_fanout_sync_confirmed": (C.c_int, [_P, C.c_int]),
    "ggrs_hip_fanout_step": (C.c_int, [_P, C.POINTER(Request), C.c_uint32, C.POINTER(C.c_uint32)]),
    "ggrs_hip_fanout_set_interval": (C.c_int, [_P, C.c_uint32]),
    "ggrs_hip_fanout_collect": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ggrs_hip_fanout_destroy": (None, [_P]),
    "ggrs_hip_fanout_last_error": (C.c_char_p, [_P]),
    "ggrs_hip_fanout_comm_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ggrs_hip_fanout_step_branches": (C.c_int, [_P, C.POINTER(BranchStep), C.POINTER(C.c_uint32)]),
    "ggrs_hip_fanout_adopt": (C.c_int, [_P, C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(Request), C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "ggrs_hip_profile_enable": (C.c_int, [_P, C.c_int]),
    "ggrs_hip_profile_read": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "ggrs_hip_profile_read_bytes": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "ggrs_hip_profile_read_launches": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]),
    "ggrs_hip_world_kernel_info": (C.c_int, [_P, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "ggrs_hip_specialise_wait": (C.c_int, [_P]),
}


# test hooks the header does not declare (ggrs_dbg_*) that the package binds with their types
DEBUG_SIGNATURES = {
    "ggrs_dbg_set_parts_grid": (C.c_int, [_P, C.c_int]),
    "ggrs_dbg_parts_launch_us": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double)]),
    "ggrs_dbg_set_query_grid": (C.c_int, [_P, C.c_int]),
    "ggrs_dbg_query_launch_us": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double)]),
    "ggrs_dbg_scatter_launch_us": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double)]),
    "ggrs_dbg_set_sort_form": (C.c_int, [_P, C.c_int]),
    "ggrs_dbg_sorted_query_launch_us": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double)]),
    "ggrs_dbg_parts_kernel_source": (C.c_int, [_P, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_int]),
}


def _preload_hip_runtime():
    """ONE HIP runtime per process.  torch wheels bundle their own libamdhip64.so (SONAME
    libamdhip64.so.7, referenced by torch as plain `libamdhip64.so`); libggrs_hip.so needs
    `libamdhip64.so.7`.  If our library is loaded before torch, the loader would map /opt/rocm's copy
    for us and torch's copy for torch -- two runtimes, and the second one to initialise sees no
    device.  Mapping torch's copy first (when torch is installed; it is not imported here) makes both
    resolve to the same file regardless of import order."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is not None and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def load_library(path: str = LIB_PATH) -> C.CDLL:
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C bevy_ggrs_amd/csrc`). "
            "bevy_ggrs_amd has no CPU fallback.")
    _preload_hip_runtime()
    lib = C.CDLL(path)
    for name, (res, args) in list(SIGNATURES.items()) + list(DEBUG_SIGNATURES.items()):
        fn = getattr(lib, name)       # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


lib = load_library()


class GgrsHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ggrs_hip error {code}: {msg}")
        self.code = code
