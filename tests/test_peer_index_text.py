"""The peer index (ggrs_hip_register_peer_index: e.bucket(key) / b.count() / b.slot(i)) checked WITHOUT a GPU on GGRS_WORLD_LAYOUT_ONLY worlds: the entry points
exist in every layer that mirrors the ABI; every seal rule and refusal answers GGRS_E_INVALID with a message naming the system and the column; the generated text
of the crowd world holds the lowering -- a bounds test, two 4-byte loads of ix_start, one of ix_slots per slot(i), plain loads -- and one-step groups; the census
and crowd kernels compile for gfx950 without scratch; and a world with peer bindings but no index, like the particles world, keeps its text byte for byte
(tests/golden/follow_world_*.hip is the text of the commit before the index existed)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import bevy_ggrs_amd as bg
import common as cm
from bevy_ggrs_amd import _ffi
from peer_index_common import CENSUS_SRC, REKEY_SRC, build_census, build_crowd
from peer_reads_common import build_follow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]
NEW_IDENTIFIERS = ("ix_start", "ix_slots", "ix_buckets", "GgrsBucket", "ixs_", "ixl_", "ixn_")          # what a world without an index does not name
USER = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) = e.bucket(e.peer(e.slot).u32(0)).count(); }"
NOP = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) += 1u; }"
DEFER = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { if (e.u32(0) == 7u) e.despawn_rollback(); }"


def layout_world(cap=600, flags=0):
    return bg.World(cap, max_depth=8, flags=bg.GGRS_WORLD_LAYOUT_ONLY | flags)


def _three(w, key_bytes=4, key_rollback=True):
    K = w.register_component("Key", key_bytes, 1, rollback=key_rollback); O = w.register_component("Out", 4, 2); H = w.register_component("Hp", 4, 1)
    w.checksum_component(O, [0, 1])
    return K, O, H


def _refused(w, *needles):
    with pytest.raises(bg.GgrsHipError) as e:
        w.generated_kernel_source()
    assert e.value.code == bg.GGRS_E_INVALID, str(e.value)
    for n in needles: assert n in str(e.value), (n, str(e.value))


def _register_refused(w, comp, word, nb, *needles, flags=0):
    d = _ffi.PeerIndexDesc(comp, word, nb, flags)
    assert w._lib.ggrs_hip_register_peer_index(w._p, C.byref(d)) == bg.GGRS_E_INVALID
    msg = w._lib.ggrs_hip_last_error(w._p).decode()
    for n in needles: assert n in msg, (n, msg)


def test_entry_points_exist_in_header_library_ctypes_mirror_cpp_backend_and_rust_shim():
    hdr = open(os.path.join(ROOT, "include", "ggrs_hip.h")).read()
    assert "typedef struct { uint32_t comp; uint32_t word; uint32_t n_buckets; uint32_t flags; } ggrs_peer_index_desc;" in hdr and "#define GGRS_HIP_ABI_VERSION 9" in hdr
    assert re.search(r"#define GGRS_PEER_INDEX_MAX_BUCKETS\s+65535u", hdr) and bg.PEER_INDEX_MAX_BUCKETS == 65535
    assert "int ggrs_hip_register_peer_index(ggrs_world* w, const ggrs_peer_index_desc* d);" in hdr
    assert "int ggrs_hip_peer_index_read(ggrs_world* w, int32_t frame, uint32_t* start, uint32_t* slots, uint64_t* n_indexed);" in hdr
    lib = C.CDLL(_ffi.LIB_PATH)
    for fn in ("ggrs_hip_register_peer_index", "ggrs_hip_peer_index_read"):
        assert hasattr(lib, fn) and fn in _ffi.SIGNATURES, fn
    assert C.sizeof(_ffi.PeerIndexDesc) == 16 and _ffi.lib.ggrs_hip_abi_version() == 9
    assert hasattr(bg.World, "register_peer_index") and hasattr(bg.World, "peer_index")
    rs = open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "ffi.rs")).read()
    assert "pub fn ggrs_hip_register_peer_index(w: *mut ggrs_world, d: *const ggrs_peer_index_desc) -> c_int;" in rs and "pub struct ggrs_peer_index_desc {" in rs
    assert "pub fn ggrs_hip_peer_index_read(w: *mut ggrs_world, frame: i32, start: *mut u32, slots: *mut u32, n_indexed: *mut u64) -> c_int;" in rs
    shim = open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "lib.rs")).read()
    assert "ffi::ggrs_hip_register_peer_index(self.raw, &d)" in shim and "ffi::ggrs_hip_peer_index_read(self.raw" in shim
    hpp = open(os.path.join(ROOT, "include", "bevy_ggrs_hip.hpp")).read()
    assert "ggrs_hip_register_peer_index(w, &d)" in hpp and "ggrs_hip_peer_index_read(w, frame, start, slots, n_indexed)" in hpp
    for words in ("ASCENDING slot order", "key >= n_buckets gives an empty bucket", "one index per world", "The kernel boundary is the only synchronisation"):
        assert words in hdr, words


def test_registration_refusals():
    w = layout_world(); K, O, H = _three(w)
    _register_refused(w, K, 0, 0, "'Key'", "n_buckets must be 1 .. 65535")
    _register_refused(w, K, 0, 65536, "'Key'", "n_buckets must be 1 .. 65535", "65536")
    _register_refused(w, K, 0, 8, "'Key'", "unknown flags", flags=1)
    _register_refused(w, K, 3, 8, "word 3 of component 0", "not registered")
    _register_refused(w, 9, 0, 8, "component 9", "not registered")
    assert w._lib.ggrs_hip_register_peer_index(w._p, None) == bg.GGRS_E_INVALID
    w.register_peer_index(K, 0, 65535)
    _register_refused(w, O, 0, 8, "already has a peer index", "'Key'", "one index per world")
    w = layout_world(); K, O, H = _three(w)
    start = (C.c_uint32 * 9)()
    assert w._lib.ggrs_hip_peer_index_read(w._p, bg.LIVE, start, None, None) == bg.GGRS_E_INVALID and b"no peer index" in w._lib.ggrs_hip_last_error(w._p)
    w.register_peer_index(K, 0, 8); w.add_custom_system(USER, [(O, 0)], name="user", peers=[(K, 0)])
    assert w._lib.ggrs_hip_peer_index_read(w._p, bg.LIVE, start, None, None) == bg.GGRS_E_NO_DEVICE


def test_e_bucket_exists_only_in_worlds_with_a_registered_index():
    w = layout_world(); K, O, H = _three(w)
    with pytest.raises(bg.GgrsHipError) as e: w.add_custom_system(USER, [(O, 0)], name="user", peers=[(K, 0)])
    assert "bucket" in str(e.value)                                        # the compiler: no member named 'bucket'


def test_seal_rules_name_the_system_and_the_column():
    # a system that uses the index and has no peer binding
    w = layout_world(); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) = e.bucket(1u).count(); }", [(O, 0)], name="user")
    _refused(w, "'user'", "'Key'", "word 0 of component 0", "has no peer binding")
    # ... registered after a writer of the key column
    w = layout_world(); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    w.add_custom_system(NOP, [(K, 0)], name="writer"); w.add_custom_system(USER, [(O, 0)], name="user", peers=[(K, 0)])
    _refused(w, "'user'", "'Key'", "system 0, registered before it, writes", "every system that uses the index is registered before every system that writes its key")
    # ... the writer may be a system that only peer-binds another column: the key column is peer binding "key" of every user
    w = layout_world(); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    w.add_custom_system(NOP, [(K, 0)], name="writer"); w.add_custom_system(USER, [(O, 0)], name="user", peers=[(H, 0)])
    _refused(w, "'user'", "'Key'", "registered before it, writes")
    # ... after another system that can despawn
    w = layout_world(); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, 0)); w.add_custom_system(USER, [(O, 0)], name="user", peers=[(K, 0)])
    _refused(w, "'user'", "'Key'", "can despawn", "every system that uses the index is registered before every other system that can despawn")
    # ... that binds the key column as its own
    w = layout_world(); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    w.add_custom_system(USER, [(O, 0), (K, 0)], name="user", peers=[(H, 0)])
    _refused(w, "'user'", "'Key'", "as its own binding 1", "share no column")
    # a key word that is not 4 bytes
    w = layout_world(); K, O, H = _three(w, key_bytes=8); w.register_peer_index(K, 0, 8)
    w.add_custom_system(USER, [(O, 0)], name="user", peers=[(H, 0)])
    _refused(w, "'Key'", "has 8 bytes", "a key is a 4-byte word")
    # a key component under a Strategy
    w = layout_world(); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    w.register_component_strategy(K, 2, 1, "__device__ void ggrs_store(const GgrsWords& t, GgrsWords& s) { s.u16(0) = (unsigned short)t.u32(0); }\n"
                                           "__device__ void ggrs_load(const GgrsWords& s, GgrsWords& t) { t.u32(0) = s.u16(0); }")
    w.add_custom_system(USER, [(O, 0)], name="user", peers=[(H, 0)])
    _refused(w, "'Key'", "Strategy")
    # ... outside rollback
    w = layout_world(); K, O, H = _three(w, key_rollback=False); w.register_peer_index(K, 0, 8)
    w.add_custom_system(USER, [(O, 0)], name="user", peers=[(H, 0)])
    _refused(w, "'Key'", "GGRS_COMP_NO_ROLLBACK")
    # an index in a world where no system uses it
    w = layout_world(); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    w.add_custom_system(NOP, [(O, 0)], name="other", peers=[(H, 0)])
    _refused(w, "'Key'", "no system of this world uses it")
    # (a world whose capacity exceeds 2^32 is refused too -- the slots are 32-bit -- but no world reaches that rule today: creation stops at 2^28 slots.  It has
    # no test; registering after seal needs a device: tests/test_gpu_peer_index.py)
    with pytest.raises(bg.GgrsHipError): layout_world(cap=(1 << 32) + 1024)


def test_the_key_is_a_peer_binding_of_every_index_user_for_the_effect_and_remote_rules_too():
    # an index user that sends an effect into the key column: the start-of-frame buckets would not be what Bevy's immediate write shows
    w = layout_world(); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) = e.bucket(1u).count(); e.send_u32(e.slot, 0, 1u); }", [(O, 0)], name="user",
                        peers=[(H, 0)], effects=[(K, 0, bg.EFFECT_ADD)])
    _refused(w, "'user'", "'Key'", "binds that column itself")
    # ... and one registered after a sender into the key column
    w = layout_world(); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.send_u32(e.slot, 0, 1u); }", [(O, 1)], name="sender", effects=[(K, 0, bg.EFFECT_ADD)])
    w.add_custom_system(USER, [(O, 0)], name="user", peers=[(H, 0)])
    _refused(w, "'Key'")
    # an index user that remotely commands the key component itself (registered AFTER a commander it is already refused as after a writer of the key)
    w = layout_world(); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) = e.bucket(1u).count(); e.send_insert(e.slot, 0); }", [(O, 0)], name="user",
                        peers=[(H, 0)], remote=[(K, bg.REMOTE_INSERT)])
    _refused(w, "'user'", "'Key'", "a remote commander does not bind a component it commands")
    w = layout_world(); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.send_insert(e.slot, 0); }", [(O, 1)], name="commander", remote=[(K, bg.REMOTE_INSERT)])
    w.add_custom_system(USER, [(O, 0)], name="user", peers=[(H, 0)])
    _refused(w, "'user'", "'Key'", "registered before it, writes")


def test_everything_peers_refuse_stays_refused():
    # a world that keeps RollbackDespawned markers
    w = layout_world(); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    w.add_custom_system(USER, [(O, 0)], name="user", peers=[(K, 0)]); w.add_custom_system(DEFER, [(H, 0)], name="defer")
    _refused(w, "RollbackDespawned markers")
    # a world that spawns on the device with e.spawn(n)
    w = layout_world(); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) = e.bucket(e.peer(e.slot).u32(0)).count(); if (e.u32(0) > 3u) e.spawn(1); }",
                        [(O, 0)], name="user", peers=[(K, 0)])
    w.add_spawn_system("__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64 k, const GgrsFrame&, const unsigned char*) { e.u32(0) = (ggrs_u32)k; }", bundle=(H,), bindings=[(H, 0)],
                       payload_stride=0xFFFFFFFF)
    _refused(w, "spawns on the device", "e.spawn(n)")
    # a world without the generated kernel
    w = layout_world(flags=bg.GGRS_WORLD_NO_GROUPS); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    w.add_custom_system(USER, [(O, 0)], name="user", peers=[(K, 0)])
    _refused(w, "need the generated request-group kernel")
    # the key column counts against GGRS_PEER_MAX_COLUMNS
    w = layout_world(); K, O, H = _three(w); w.register_peer_index(K, 0, 8)
    wide = [w.register_component(f"W{k}", 4, 8) for k in range(2)]
    w.add_custom_system(USER, [(O, 0)], name="user", peers=[(wide[0], k) for k in range(8)])
    w.add_custom_system(NOP, [(O, 1)], name="more", peers=[(wide[1], k) for k in range(8)])
    _refused(w, "17 distinct peer-bound columns", "GGRS_PEER_MAX_COLUMNS")


def test_the_generated_text_of_the_crowd_world_holds_the_lowering_and_one_step_groups():
    w = layout_world(8400); build_crowd(w, 255, 257)
    src = w.generated_kernel_source()
    # the argument block: three optional fields, next to the view's
    for decl in ("const ggrs_u32* ix_start;", "const ggrs_u32* ix_slots;", "ggrs_u32 ix_buckets;", "const ggrs_u64* pv_vis;"): assert decl in src, decl
    assert "const unsigned char* pv_col[3];" in src                        # Pos.x, Pos.y and the key column: a peer-bound column of the world
    # the lowering: a bounds test on the key, two 4-byte loads of ix_start, one 4-byte load of ix_slots per slot(i) -- plain loads, no modifier
    assert "if (key < ixn_) {" in src
    assert "s0 = *(const GGRS_G ggrs_u32*)(ixs_ + (ggrs_u64)key * 4ul), s1 = *(const GGRS_G ggrs_u32*)(ixs_ + (ggrs_u64)key * 4ul + 4ul);" in src
    assert "return i < n_ ? (ggrs_u64)*(const GGRS_G ggrs_u32*)(sl_ + ((ggrs_u64)b_ + i) * 4ul) : ~0ull;" in src
    bucket_text = src[src.index("struct GgrsBucket {"):src.index("struct GgrsEntity")]
    assert "__builtin_nontemporal" not in bucket_text and "volatile" not in bucket_text and "atomic" not in bucket_text
    # only the system that names `bucket` gets the arrays; the others see an index of 0 buckets
    assert src.count("ent.ixs_ = (unsigned long)a.ix_start; ent.ixl_ = (unsigned long)a.ix_slots; ent.ixn_ = a.ix_buckets;") == 1
    # one AdvanceWorld per launch: the per-step arrays of the argument block have one entry
    assert re.search(r"ggrs_u32 dt_bits\[1\];", src) and re.search(r"int step_frame\[1\];", src)
    # a specialised copy keeps the index as arguments
    steady = w.generated_kernel_source(steady=True)
    assert "a.ix_start" in steady and "a.ix_buckets" in steady and "a.pv_col[2]" in steady


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")
@pytest.mark.parametrize("which", ["census", "crowd"])
def test_the_worlds_compile_for_gfx950_without_scratch(which):
    w = layout_world(8400)
    if which == "census": build_census(w, 300)
    else: build_crowd(w, 255, 257)
    for steady in (False, True):
        src = w.generated_kernel_source(steady=steady, compile=True)          # ggrs_hip_generated_kernel_source(compile=1): builds for gfx950, no device needed
        rtc = C.CDLL("libhiprtc.so")
        prog = C.c_void_p()
        assert rtc.hiprtcCreateProgram(C.byref(prog), src.encode(), b"k.hip", 0, None, None) == 0
        assert rtc.hiprtcCompileProgram(prog, len(OPTS), (C.c_char_p * len(OPTS))(*OPTS)) == 0
        n = C.c_size_t(); rtc.hiprtcGetCodeSize(prog, C.byref(n)); code = C.create_string_buffer(n.value); rtc.hiprtcGetCode(prog, code)
        with tempfile.NamedTemporaryFile(suffix=".hsaco") as f:
            f.write(code.raw); f.flush()
            notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
            asm = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", f.name], capture_output=True, text=True, check=True).stdout
        res = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|sgpr_count):\s+(\d+)", notes)}
        print(which, "steady" if steady else "generic", res)
        assert res.get("private_segment_fixed_size") == 0 and res.get("vgpr_spill_count") == 0 and res.get("vgpr_count") <= 64, res
        assert "scratch_" not in asm and "buffer_wbl2" not in asm and "buffer_inv" not in asm       # no scratch access; the kernel boundary is the only synchronisation


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf")), reason="no hipcc / llvm-readelf")
def test_the_build_kernels_compile_without_scratch():
    csrc = os.path.join(ROOT, "bevy_ggrs_amd", "csrc")
    flags = re.search(r"^HIPFLAGS \?= (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).replace("$(ARCH)", "gfx950").split()
    with tempfile.NamedTemporaryFile(suffix=".hsaco") as f:
        subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--offload-device-only", "--no-gpu-bundle-output", "-c", os.path.join(csrc, "ggrs_hip.hip"), "-o", f.name], check=True, capture_output=True)
        notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
    seen = set()
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        kind = next((k for k in ("k_ix_hist", "k_ix_scan", "k_ix_scatter", "k_ix_bounds", "k_ix_small") if k in name), None)
        if not kind: continue
        res = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|group_segment_fixed_size|vgpr_count):\s+(\d+)", blk)}
        print(name, res)
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0 and res["vgpr_count"] <= 64 and res["group_segment_fixed_size"] <= 12288, (name, res)
        seen.add(kind)
    assert seen == {"k_ix_hist", "k_ix_scan", "k_ix_scatter", "k_ix_bounds", "k_ix_small"}


def test_worlds_without_an_index_keep_their_text():
    """The follow world of the peer-read tests -- peer bindings, no index -- generates the text of the commit before the index existed, byte for byte
    (tests/golden/follow_world_*.hip); the particles world's text is the committed headline text."""
    for form, steady in (("generic", False), ("steady", True)):
        w = layout_world(); build_follow(w)
        src = w.generated_kernel_source(steady=steady)
        assert src == open(os.path.join(ROOT, "tests", "golden", f"follow_world_{form}.hip")).read(), form
        for ident in NEW_IDENTIFIERS + ("bucket",): assert ident not in src, ident
        w = bg.World(1_000_000, max_depth=9, flags=bg.GGRS_WORLD_LAYOUT_ONLY); cm.build_particles(w)
        assert w.generated_kernel_source(steady=steady) == open(os.path.join(ROOT, "docs", "generated", f"headline_{form}.hip")).read(), form
    assert getattr(_ffi.lib, "ggrs_hip_register_peer_index")              # (on the parent the symbol is missing: this test fails there too)
