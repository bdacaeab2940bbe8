"""The numpy model of the checksum parts (tests/checksum_parts_common.py model_parts) against hand-written cases computed with the plain-Python SeaHasher, and
against the C++ oracle's Checksum frame by frame -- what guards the model the GPU tests compare the device with -- and the agreement of include/ggrs_hip.h, the
ctypes mirror and rust/bevy_ggrs_hip/src/ffi.rs on the two structs, the three kinds and the three symbols."""
import ctypes as C
import os
import re

import numpy as np

import bevy_ggrs_amd as bg
import checksum_parts_common as cp
import common as cm
from bevy_ggrs_amd import _ffi
from oracle import oracle_np as onp
from oracle.binding import FLAT, OracleWorld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64


# ---- the expectation, entity by entity, with the stream hasher alone
def py_inner(fields):
    h = onp.SeaHasher()
    for v, nb in fields: h.write(int(v).to_bytes(nb, "little"))
    return h.finish()


def py_part(entities):
    """entities: [(slot, [(value, bytes) ..])] -> the component's ChecksumPart."""
    x = 0
    for slot, fields in entities: x ^= onp.SeaHasher().write_u64(slot).write_u64(py_inner(fields)).finish()
    return onp.SeaHasher().write_u64(x).finish()


def rec(n, alive, present, words, res=None):
    return {"len": n, "alive": np.array(alive, dtype=bool), "present": {c: np.array(p, dtype=bool) for c, p in present.items()},
            "words": {k: np.asarray(v) for k, v in words.items()}, "res": res or {}}


def test_an_empty_world_has_the_entity_part_alone():
    m = cp.model_parts(rec(0, [], {}, {}), cp.Specs())
    assert list(m["parts"]) == ["Entity"] and m["parts"]["Entity"] == onp.entity_checksum(0, 0) == m["checksum"] and m["active"] == 0 and m["len"] == 0


def test_a_component_nobody_holds_is_sea_one_of_zero():
    specs = cp.Specs([("X", 0, [(0, 4)])])
    m = cp.model_parts(rec(3, [1, 1, 0], {0: [0, 0, 1]}, {(0, 0): np.array([5, 6, 7], dtype=U32)}), specs)      # the only holder is dead
    zero = onp.SeaHasher().write_u64(0).finish()
    assert zero != 0 and m["parts"]["X"] == zero and m["counts"] == {"X": 0, "Entity": 2}
    assert m["checksum"] == zero ^ onp.entity_checksum(2, 3)


def test_one_entity_of_each_word_width():
    specs = cp.Specs([("B1", 0, [(0, 1)]), ("B2", 1, [(1, 2), (0, 2)]), ("B4", 2, [(0, 4), (1, 4), (2, 4)]), ("B8", 3, [(0, 8)])])
    words = {(0, 0): np.array([0xAB], dtype=U8), (1, 0): np.array([0x1234], dtype=U16), (1, 1): np.array([0xFFEE], dtype=U16),
             (2, 0): np.array([1], dtype=U32), (2, 1): np.array([0x80000000], dtype=U32), (2, 2): np.array([3], dtype=U32), (3, 0): np.array([(1 << 63) | 9], dtype=U64)}
    m = cp.model_parts(rec(1, [1], {c: [1] for c in range(4)}, words), specs)
    assert m["parts"]["B1"] == py_part([(0, [(0xAB, 1)])])
    assert m["parts"]["B2"] == py_part([(0, [(0xFFEE, 2), (0x1234, 2)])])                              # the spec's order, not the component's
    assert m["parts"]["B4"] == py_part([(0, [(1, 4), (0x80000000, 4), (3, 4)])])
    assert m["parts"]["B8"] == py_part([(0, [((1 << 63) | 9, 8)])])
    assert m["parts"]["Entity"] == onp.entity_checksum(1, 1) and all(m["counts"][k] == 1 for k in m["counts"])
    # the words cross the 8-byte boundary of the stream: 2 + 4 + 4 bytes
    specs = cp.Specs([("M", 0, [(0, 4), (1, 4), (2, 4)])])
    w3 = {(0, k): np.array([10 + k, 20 + k], dtype=U32) for k in range(3)}
    m = cp.model_parts(rec(2, [1, 1], {0: [1, 1]}, w3), specs)
    assert m["parts"]["M"] == py_part([(0, [(10, 4), (11, 4), (12, 4)]), (1, [(20, 4), (21, 4), (22, 4)])]) and m["counts"]["M"] == 2


def test_a_slot_beyond_len_is_dead_whatever_its_alive_bit_says():
    specs = cp.Specs([("X", 0, [(0, 4)])])
    w = {(0, 0): np.array([5, 6, 7], dtype=U32)}
    cut = cp.model_parts(rec(2, [1, 1, 1], {0: [1, 1, 1]}, w), specs)                                  # arrays of three slots, len 2
    assert cut["parts"]["X"] == py_part([(0, [(5, 4)]), (1, [(6, 4)])]) and cut["active"] == 2 and cut["parts"]["Entity"] == onp.entity_checksum(2, 2)
    whole = cp.model_parts(rec(3, [1, 1, 1], {0: [1, 1, 1]}, w), specs)
    assert whole["parts"]["X"] != cut["parts"]["X"] and whole["active"] == 3


def test_planted_bytes_under_a_dead_slot_and_an_absent_component_move_nothing():
    specs = cp.Specs([("X", 0, [(0, 4)]), ("Y", 1, [(0, 8)])])
    a = rec(3, [1, 0, 1], {0: [1, 1, 0], 1: [1, 1, 1]}, {(0, 0): np.array([1, 2, 3], dtype=U32), (1, 0): np.array([4, 5, 6], dtype=U64)})
    b = rec(3, [1, 0, 1], {0: [1, 1, 0], 1: [1, 1, 1]}, {(0, 0): np.array([1, 999, 777], dtype=U32), (1, 0): np.array([4, 555, 6], dtype=U64)})
    ma, mb = cp.model_parts(a, specs), cp.model_parts(b, specs)
    assert ma == mb and ma["counts"] == {"X": 1, "Y": 2, "Entity": 2}
    b["words"][(1, 0)][2] = 60                                                                         # a live holder's word does move its part, and only it
    mc = cp.model_parts(b, specs)
    assert [k for k in ma["parts"] if ma["parts"][k] != mc["parts"][k]] == ["Y"]


def test_a_despawn_and_a_spawn_move_the_entity_part_through_active_and_len_only():
    specs = cp.Specs([("X", 0, [(0, 4)])])
    a = rec(3, [1, 1, 1], {0: [1, 1, 0]}, {(0, 0): np.array([1, 2, 3], dtype=U32)})
    b = rec(4, [1, 1, 0, 1], {0: [1, 1, 0, 0]}, {(0, 0): np.array([1, 2, 3, 4], dtype=U32)})          # slot 2 (no X) despawned, slot 3 (no X) spawned
    ma, mb = cp.model_parts(a, specs), cp.model_parts(b, specs)
    assert ma["parts"]["X"] == mb["parts"]["X"] and (ma["active"], mb["active"]) == (3, 3)
    assert ma["parts"]["Entity"] == onp.entity_checksum(3, 3) and mb["parts"]["Entity"] == onp.entity_checksum(3, 4) and ma["parts"]["Entity"] != mb["parts"]["Entity"]


def test_resource_parts_hash_the_chosen_words_at_their_width():
    specs = cp.Specs([], [("Clock", 0, 4, [1, 0]), ("Wide", 2, 8, [0])])
    m = cp.model_parts(rec(0, [], {}, {}, {0: [5, 77], 2: [(1 << 40) + 3]}), specs)
    assert list(m["parts"]) == ["Entity", "Clock", "Wide"]
    assert m["parts"]["Clock"] == py_inner([(77, 4), (5, 4)]) and m["parts"]["Wide"] == py_inner([((1 << 40) + 3, 8)]) and m["counts"]["Clock"] == 0
    assert m["checksum"] == m["parts"]["Entity"] ^ m["parts"]["Clock"] ^ m["parts"]["Wide"]


def test_a_numpy_hasher_stands_in_for_user_source():
    def hasher(words, slots): return onp.np_inner_hash_fields([(words[1], 4)]) ^ U64(0x55) ^ slots
    specs = cp.Specs([("X", 0, hasher)])
    m = cp.model_parts(rec(2, [1, 1], {0: [1, 1]}, {(0, 0): np.array([1, 2], dtype=U32), (0, 1): np.array([8, 9], dtype=U32)}), specs)
    x = 0
    for s, v in ((0, 8), (1, 9)): x ^= onp.SeaHasher().write_u64(s).write_u64(py_inner([(v, 4)]) ^ 0x55 ^ s).finish()
    assert m["parts"]["X"] == onp.SeaHasher().write_u64(x).finish()


# ---- the model's fold is the oracle's Checksum, frame by frame
def _scripted(w, comps, specs, edits):
    """Save f (the model over the arrays recorded right before it must fold to the oracle's checksum), a host edit, Advance -- then two frames once more behind a Load."""
    w.set_depth(8); w.set_confirmed(0)
    seen = 0
    for f in range(6):
        r = cp.record_words(w, comps)
        (cs,) = w.handle_requests([bg.SaveGameState(f)])
        m = cp.model_parts(r, specs)
        assert m["checksum"] == cs, (f, m)
        assert m["active"] == w.active_count() and m["len"] == w.len
        seen += 1
        if f < len(edits) and edits[f]: edits[f]()
        w.handle_requests([bg.AdvanceFrame((0,))])
    w.handle_requests([bg.LoadGameState(3), bg.AdvanceFrame((0,))])
    r = cp.record_words(w, comps)
    (cs,) = w.handle_requests([bg.SaveGameState(4)])
    assert cp.model_parts(r, specs)["checksum"] == cs
    return seen + 1


def test_the_models_fold_equals_the_oracles_checksum_particles():
    n = 300
    w = OracleWorld(n + 64, 8, FLAT)
    T, V, L = cm.build_particles(w)
    vel, ttl = cm.synthetic_particles(n, ttl="despawn")                                                # Ttl 1 .. 300: entities die from the first frame on
    cm.spawn_particles(w, (T, V, L), n, vel, ttl)
    specs = cp.Specs([("Transform", T, [(0, 4), (1, 4), (2, 4)]), ("Velocity", V, [(0, 4), (1, 4), (2, 4)])])
    edits = [None, lambda: w.despawn(7), lambda: w.remove_component(V, 9), lambda: cm.spawn_particles(w, (T, V, L), 5, vel[:5], ttl[:5] + U64(50)), lambda: w.despawn(n + 2)]
    assert _scripted(w, [(T, 10), (V, 3)], specs, edits) == 7
    w.close()


def test_the_models_fold_equals_the_oracles_checksum_every_word_width():
    n = 200
    w = OracleWorld(n + 16, 8, FLAT)
    A = w.register_component("A", 1, 2); B = w.register_component("B", 2, 2); H = w.register_component("H", 4, 1); Q = w.register_component("Q", 8, 1)
    N = w.register_component("Nobody", 4, 1); Z = w.register_component("Unhashed", 4, 1)
    w.checksum_component(A, [1, 0]); w.checksum_component(B, [0, 1]); w.checksum_component(H, [0]); w.checksum_component(Q, [0]); w.checksum_component(N, [0])
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, bg.DESPAWN_IMMEDIATE))       # entities die as H reaches 0
    i = np.arange(n, dtype=np.int64)
    w.spawn(n, {A: [(i % 251).astype(U8), (i * 3 % 256).astype(U8)], B: [(i * 77 % 65536).astype(U16), (65535 - i).astype(U16)], H: [(1 + i % 7).astype(U32)],
                Q: [(i.astype(U64) << U64(35)) + U64(1)], Z: [i.astype(U32)]})
    for k in range(0, n, 3): w.remove_component(B, k)
    specs = cp.Specs([("A", A, [(1, 1), (0, 1)]), ("B", B, [(0, 2), (1, 2)]), ("H", H, [(0, 4)]), ("Q", Q, [(0, 8)]), ("Nobody", N, [(0, 4)])])
    edits = [lambda: w.upload_word(Q, 0, 11, np.array([(1 << 64) - 1], dtype=U64)), lambda: w.despawn(13), lambda: w.upload_word(Z, 0, 0, np.array([99], dtype=U32)),
             lambda: w.insert_component(B, 6, np.array([1, 2], dtype=U16)), lambda: w.spawn(2, {A: [np.array([1, 2], dtype=U8), np.array([3, 4], dtype=U8)], H: [np.array([9, 9], dtype=U32)]})]
    assert _scripted(w, [(A, 2), (B, 2), (H, 1), (Q, 1), (N, 1)], specs, edits) == 7
    w.close()


# ---- header, ctypes and ffi.rs agree
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggrs_hip.h")).read(), flags=re.S)


def test_the_header_declares_the_calls_the_structs_and_the_kinds():
    h = _header()
    assert re.search(r"int ggrs_hip_checksum_parts\(ggrs_world\* w, int32_t frame, ggrs_parts_report\* report, ggrs_checksum_part\* parts, uint32_t max_parts\);", h)
    assert re.search(r"int ggrs_hip_checksum_parts_block\(ggrs_world\* w, const void\* block_dev, ggrs_parts_report\* report, ggrs_checksum_part\* parts, uint32_t max_parts\);", h)
    assert re.search(r"typedef struct \{ uint32_t kind; uint32_t id; uint64_t value; uint64_t n_hashed; \} ggrs_checksum_part;", h)
    assert re.search(r"typedef struct \{ uint64_t len; uint64_t active; uint64_t checksum_lo; uint64_t checksum_hi; uint32_t n_parts; \} ggrs_parts_report;", h)
    for name, v in (("COMPONENT", 0), ("ENTITY", 1), ("RESOURCE", 2)): assert re.search(r"#define GGRS_PART_%s\s+%du\b" % (name, v), h)
    assert re.search(r"#define GGRS_HIP_ABI_VERSION 9\b", h) and _ffi.lib.ggrs_hip_abi_version() == 9          # new functions only: the version stays
    assert "an export of per-component ChecksumParts" not in open(os.path.join(ROOT, "include", "ggrs_hip.h")).read()


def test_the_three_symbols_are_bound_and_the_structs_agree():
    assert (_ffi.PART_COMPONENT, _ffi.PART_ENTITY, _ffi.PART_RESOURCE) == (0, 1, 2)
    assert C.sizeof(_ffi.ChecksumPart) == 24 and C.sizeof(_ffi.PartsReport) == 40
    assert [f[0] for f in _ffi.ChecksumPart._fields_] == ["kind", "id", "value", "n_hashed"]
    assert [f[0] for f in _ffi.PartsReport._fields_] == ["len", "active", "checksum_lo", "checksum_hi", "n_parts"]
    for name in ("ggrs_hip_checksum_parts", "ggrs_hip_checksum_parts_block"):
        assert name in _ffi.SIGNATURES and getattr(_ffi.lib, name).argtypes == _ffi.SIGNATURES[name][1]
    assert _ffi.lib.ggrs_dbg_set_parts_grid.argtypes == [C.c_void_p, C.c_int] and _ffi.lib.ggrs_dbg_set_parts_grid.restype == C.c_int
    assert _ffi.MAX_PARTS == 32 + 1 + 8
    rs = open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "ffi.rs")).read()
    assert re.search(r"pub struct ggrs_checksum_part \{\s*pub kind: u32,\s*pub id: u32,\s*pub value: u64,\s*pub n_hashed: u64,\s*\}", rs)
    assert re.search(r"pub struct ggrs_parts_report \{\s*pub len: u64,\s*pub active: u64,\s*pub checksum_lo: u64,\s*pub checksum_hi: u64,\s*pub n_parts: u32,\s*\}", rs)
    for name, v in (("COMPONENT", 0), ("ENTITY", 1), ("RESOURCE", 2)): assert re.search(r"pub const GGRS_PART_%s: u32 = %d;" % (name, v), rs)


def test_the_kernel_generated_for_a_user_written_hasher_builds_for_gfx950():
    """A world with a user-written hasher hashes its parts with a generated kernel (only generated code can run the user's source): its text holds the device
    prelude, the shared accumulation of the static kernel, the hasher's namespace as the request-group kernel has it, and one arm per checksum spec; hiprtc builds
    it for gfx950 on any host.  The request-group kernel's own text does not change with it (tests/test_generated_golden.py)."""
    w = bg.World(1000, max_depth=4, flags=bg.GGRS_WORLD_LAYOUT_ONLY)
    X = w.register_component("X", 4, 4); Y = w.register_component("Y", 2, 2); Z = w.register_component("Z", 8, 1); B = w.register_component("B", 1, 1)
    hasher = "__device__ ggrs_u64 ggrs_hash(const GgrsComponent& c) { GgrsHasher h; h.write_u32(c.u32(0) ^ (c.u32(1) * 3u)); h.write_u8(c.u8(3) & 1); return h.finish() ^ 0x55ull ^ c.slot; }"
    w.checksum_component_custom(X, hasher); w.checksum_component(Y, [1, 0]); w.checksum_component(Z, [0]); w.checksum_component(B, [0])
    need = C.c_uint64(0)
    assert _ffi.lib.ggrs_dbg_parts_kernel_source(w._p, None, 0, C.byref(need), 0) == 0
    buf = C.create_string_buffer(need.value)
    rc = _ffi.lib.ggrs_dbg_parts_kernel_source(w._p, buf, need.value, C.byref(need), 1)
    assert rc == 0, _ffi.lib.ggrs_hip_last_error(w._p).decode()
    src = buf.value.decode()
    tick = w.generated_kernel_source()
    ns = 'namespace ggrs_hash_0 {\n#line 1 "checksum_X"\n' + hasher + "\n}\n"
    assert ns in src and ns in tick                                                                     # the namespaces exactly as the request-group kernel has them
    assert 'extern "C" __global__ __launch_bounds__(256) void ggrs_jit_parts(PartsArgs a)' in src and "ggrs_jit_tick" not in src
    body = src[src.index("void ggrs_jit_parts("):]
    assert body.count("parts_put(row, a.n_cks,") == 4 and body.count("ggrs_hash_0::ggrs_hash(cv)") == 1 and body.count("cv.w[") == 4 and body.count("st.write(") == 4
    assert body.index("221184ull") > 0 and ", 2u, e), 2u), 2u);" in body and ", 8u, e), 8u), 8u);" in body and ", 1u, e), 1u), 1u);" in body      # every width, literal offsets
    for name in ("parts_rows_clear", "parts_rows_flush", "struct PartsArgs", "sea_pair", "wave_xor", "struct GgrsHasher"): assert name in src, name
    shared = open(os.path.join(ROOT, "bevy_ggrs_amd", "csrc", "parts_shared.hpp")).read()
    assert "GGRS_SHARED_CODE(" in shared and "#pragma" not in shared and "#include" not in shared         # one text for the static and the generated kernel
    ker = open(os.path.join(ROOT, "bevy_ggrs_amd", "csrc", "kernels.hpp")).read()
    assert '#include "parts_shared.hpp"' in ker and "void k_parts_hash(PartsArgs a)" in ker and "void k_parts_finish(PartsFinArgs f)" in ker


def test_the_python_surface():
    a = bg.ChecksumParts(parts={"X": 1, "Entity": 2, "Clock": 3}, counts={"X": 4, "Entity": 5, "Clock": 0}, len=6, active=5, checksum=0)
    b = bg.ChecksumParts(parts={"X": 1, "Entity": 9, "Clock": 3}, counts={"X": 4, "Entity": 5, "Clock": 0}, len=7, active=5, checksum=0)
    assert a.differing(a) == [] and a.differing(b) == ["Entity"] == b.differing(a)
    assert "Entity" in str(a) and "len 6" in str(a) and "X" in str(a)
    from bevy_ggrs_amd.session import MismatchedChecksum
    assert not hasattr(MismatchedChecksum(3, [1]), "parts") and MismatchedChecksum(3, [1], {}, {1: (a, b)}).parts[1][0] is a
    w = bg.World(64, max_depth=4, flags=bg.GGRS_WORLD_LAYOUT_ONLY)                                      # a layout-only world: refused with a message
    rep, arr = _ffi.PartsReport(), (_ffi.ChecksumPart * _ffi.MAX_PARTS)()
    assert _ffi.lib.ggrs_hip_checksum_parts(w._p, 0, C.byref(rep), arr, _ffi.MAX_PARTS) == bg.GGRS_E_INVALID
    assert b"layout-only" in _ffi.lib.ggrs_hip_last_error(w._p)
