"""Peer bindings (ggrs_hip_add_custom_system_peers: a user-written system reads OTHER entities through e.peer(slot)), checked WITHOUT a GPU on
GGRS_WORLD_LAYOUT_ONLY worlds: the entry point exists in every layer that mirrors the ABI; every rule and refusal of include/ggrs_hip.h answers
GGRS_E_INVALID with its message; the follow world's generated text holds the gather, compiles for gfx950 and needs no scratch; the text of a world
without peer bindings is what it was."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import bevy_ggrs_amd as bg
import common as cm
from bevy_ggrs_amd import _ffi
from peer_reads_common import CHILD_SRC, FOLLOW_SRC, INTEGRATE_SRC, build_follow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]
NEW_IDENTIFIERS = ("pv_col", "pv_vis", "pv_len")      # what no world without peer bindings names (an effect world has a view of its own: "pv_", "GgrsPeer")
NOP = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) += 1u; }"
READ = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { const GgrsPeer p = e.peer(e.u64(1)); if (p.ok()) e.u32(0) = p.u32(0); }"


def layout_world(cap=600, flags=0):
    return bg.World(cap, max_depth=8, flags=bg.GGRS_WORLD_LAYOUT_ONLY | flags)


def test_entry_point_exists_in_header_library_ctypes_and_rust_shim():
    hdr = open(os.path.join(ROOT, "include", "ggrs_hip.h")).read()
    assert re.search(r"int ggrs_hip_add_custom_system_peers\(ggrs_world\* w, const ggrs_custom_system_desc\* desc,\s*const ggrs_peer_binding\* peers, uint32_t n_peers\);", hdr)
    assert "#define GGRS_PEER_MAX_BINDINGS 8" in hdr and "ggrs_peer_binding;" in hdr and "#define GGRS_HIP_ABI_VERSION 9" in hdr
    assert hasattr(C.CDLL(_ffi.LIB_PATH), "ggrs_hip_add_custom_system_peers") and "ggrs_hip_add_custom_system_peers" in _ffi.SIGNATURES
    assert C.sizeof(_ffi.PeerBinding) == 8
    rs = open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "ffi.rs")).read()
    assert "pub fn ggrs_hip_add_custom_system_peers(w: *mut ggrs_world, desc: *const ggrs_custom_system_desc, peers: *const ggrs_peer_binding, n_peers: u32) -> c_int;" in rs
    assert "ffi::ggrs_hip_add_custom_system_peers(" in open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "lib.rs")).read()
    assert "ggrs_hip_add_custom_system_peers(w, d, peers, n_peers)" in open(os.path.join(ROOT, "include", "bevy_ggrs_hip.hpp")).read()
    # the semantics, in the header's words
    for words in ("A peer read returns the value the word had at the start of the frame, before any system of this AdvanceWorld ran.",
                  "Entities spawned in this frame are not visible.", "is still visible this frame"):
        assert words in hdr, words
    assert "no cross-entity reads" not in hdr


def test_zero_peers_is_the_plain_entry_point():
    a, b = layout_world(), layout_world()
    for w, peers in ((a, ()), (b, None)):
        A = w.register_component("A", 4, 1); w.checksum_component(A, [0])
        if peers is None: w.add_custom_system(NOP, [(A, 0)])
        else:
            d = _ffi.CustomSystemDesc(); d.name, d.source, d.n_bindings = b"custom", NOP.encode(), 1; d.comp[0], d.word[0] = A, 0
            w._check(w._lib.ggrs_hip_add_custom_system_peers(w._p, C.byref(d), None, 0))
    assert a.generated_kernel_source() == b.generated_kernel_source() and "GgrsPeer" not in a.generated_kernel_source()


def _refused(w, *needles):
    with pytest.raises(bg.GgrsHipError) as e:
        w.generated_kernel_source()
    assert e.value.code == bg.GGRS_E_INVALID, str(e.value)
    for n in needles: assert n in str(e.value), (n, str(e.value))


def _two(w):
    A = w.register_component("Alpha", 4, 1); L = w.register_component("Link", 8, 1)
    w.checksum_component(A, [0])
    return A, L


def test_rule_peer_system_precedes_every_writer_of_a_column_it_reads():
    w = layout_world(); A, L = _two(w)
    B = w.register_component("Beta", 4, 1)
    w.add_custom_system(NOP, [(A, 0)], name="writer")
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { const GgrsPeer p = e.peer(e.u64(1)); if (p.ok()) e.u32(0) = p.u32(0); }",
                        [(B, 0), (L, 0)], name="reader", peers=[(A, 0)])
    _refused(w, "'reader'", "'Alpha'", "word 0", "writes", "registered before every system that writes a column it peer-reads")
    # a built-in writer counts as well
    w = layout_world(); A, L = _two(w); B = w.register_component("Beta", 4, 1)
    w.add_system(bg.SYS_ADD_U32, comp=(A,), word=(0,), iparam=(1,))
    w.add_custom_system(READ, [(B, 0), (L, 0)], name="reader", peers=[(A, 0)])
    _refused(w, "'reader'", "'Alpha'", "writes")
    # the other order is accepted
    w = layout_world(); A, L = _two(w); B = w.register_component("Beta", 4, 1)
    w.add_custom_system(READ, [(B, 0), (L, 0)], name="reader", peers=[(A, 0)])
    w.add_system(bg.SYS_ADD_U32, comp=(A,), word=(0,), iparam=(1,))
    assert "GgrsPeer" in w.generated_kernel_source()


def test_rule_peer_system_precedes_every_other_system_that_can_despawn():
    for first in ("builtin", "custom"):
        w = layout_world(); A, L = _two(w); B = w.register_component("Beta", 4, 1); H = w.register_component("Hp", 4, 1)
        if first == "builtin": w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, 0))
        else: w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { if (e.u32(0) == 0u) e.despawn(); }", [(H, 0)], name="reaper")
        w.add_custom_system(READ, [(B, 0), (L, 0)], name="reader", peers=[(A, 0)])
        _refused(w, "'reader'", "'Alpha'", "can despawn", "registered before every other system that can despawn")


def test_rule_own_and_peer_bindings_share_no_column():
    w = layout_world(); A, L = _two(w)
    w.add_custom_system(READ, [(A, 0), (L, 0)], name="reader", peers=[(A, 0)])
    _refused(w, "'reader'", "'Alpha'", "share no column")


def test_refusals_of_the_first_version():
    # a peer-bound component under a Strategy
    w = layout_world(); A, L = _two(w); B = w.register_component("Beta", 4, 1)
    w.register_component_strategy(A, 2, 1, "__device__ void ggrs_store(const GgrsWords& t, GgrsWords& s) { s.u16(0) = (unsigned short)t.u32(0); }\n"
                                           "__device__ void ggrs_load(const GgrsWords& s, GgrsWords& t) { t.u32(0) = s.u16(0); }")
    w.add_custom_system(READ, [(B, 0), (L, 0)], name="reader", peers=[(A, 0)])
    _refused(w, "'reader'", "'Alpha'", "Strategy")
    # a non-rollback peer-bound component
    w = layout_world(); A, L = _two(w); N = w.register_component("Mesh", 4, 1, rollback=False)
    w.add_custom_system(READ, [(A, 0), (L, 0)], name="reader", peers=[(N, 0)])
    _refused(w, "'reader'", "'Mesh'", "GGRS_COMP_NO_ROLLBACK")
    # a world that keeps RollbackDespawned markers
    w = layout_world(); A, L = _two(w); B = w.register_component("Beta", 4, 1); H = w.register_component("Hp", 4, 1)
    w.add_custom_system(READ, [(B, 0), (L, 0)], name="reader", peers=[(A, 0)])
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, bg.DESPAWN_ROLLBACK))
    _refused(w, "RollbackDespawned markers")
    # a world that spawns on the device with e.spawn(n)
    w = layout_world(); A, L = _two(w); B = w.register_component("Beta", 4, 1)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { const GgrsPeer p = e.peer(e.u64(1)); if (p.ok()) e.spawn(1); }",
                        [(B, 0), (L, 0)], name="reader", peers=[(A, 0)])
    w.add_spawn_system("__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64 k, const GgrsFrame&, const unsigned char*) { e.u32(0) = (ggrs_u32)k; }", bundle=(A,), bindings=[(A, 0)],
                       payload_stride=0xFFFFFFFF)
    _refused(w, "spawns on the device", "e.spawn(n)")
    # worlds without the generated kernel
    for flags in (bg.GGRS_WORLD_NO_GROUPS, bg.GGRS_WORLD_UNFUSED):
        w = layout_world(flags=flags); A, L = _two(w); B = w.register_component("Beta", 4, 1)
        w.add_custom_system(READ, [(B, 0), (L, 0)], name="reader", peers=[(A, 0)])
        _refused(w, "need the generated request-group kernel")
    # bad arguments
    w = layout_world(); A, L = _two(w)
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_custom_system(READ, [(A, 0), (L, 0)], peers=[(7, 0)])
    assert e.value.code == bg.GGRS_E_INVALID and "peer binding 0" in str(e.value)
    with pytest.raises(ValueError):
        w.add_custom_system(READ, [(A, 0), (L, 0)], peers=[(A, 0)] * 9)


def test_no_generated_kernel_knob_is_refused(monkeypatch):
    monkeypatch.setenv("GGRS_TICK_JIT", "0")
    w = layout_world(); A, L = _two(w); B = w.register_component("Beta", 4, 1)
    w.add_custom_system(READ, [(B, 0), (L, 0)], name="reader", peers=[(A, 0)])
    _refused(w, "need the generated request-group kernel", "GGRS_TICK_JIT=0")


def follow_world(cap=600, with_spawn=False):
    w = layout_world(cap)
    build_follow(w, with_spawn=with_spawn)
    return w


def test_follow_world_text_holds_the_gather_and_one_step_groups():
    src = follow_world().generated_kernel_source()
    body = src.split('extern "C" __global__')[1]
    # the view's base pointers are in the argument block, the two peer-bound columns only
    assert re.search(r"const unsigned char\* pv_col\[2\];", src) and "const ggrs_u64* pv_vis;" in src and "ggrs_u64 pv_len;" in src
    # e.peer(slot): bounds test against the view's len, one load of the visibility word and a bit test; per accessor one load from the linear column
    assert "if (s < pv_.len) p.ok_ = (*(const GGRS_G ggrs_u64*)(pv_.vis + (s >> 6) * 8ul) >> (s & 63ull)) & 1ull;" in src
    assert "case 4: return *(const GGRS_G ggrs_u32*)(v_.col[j] + s_ * 4ul);" in src and "if (!ok_) return 0ull;" in src
    assert "ent.pv_.len = a.pv_len; ent.pv_.vis = (unsigned long)a.pv_vis;" in body
    assert "ent.pv_.col[0] = (unsigned long)a.pv_col[0]; ent.pv_.wb[0] = 4u;" in body and "ent.pv_.col[1] = (unsigned long)a.pv_col[1]; ent.pv_.wb[1] = 4u;" in body
    # one AdvanceWorld per launch: every per-step array of the argument block has one element
    assert re.search(r"ggrs_u32 dt_bits\[1\];", src) and re.search(r"int step_frame\[1\];", src)
    # a specialised copy keeps the view's pointers as arguments
    steady = follow_world().generated_kernel_source(steady=True)
    assert "a.pv_len" in steady and "a.pv_col[1]" in steady


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="no llvm-readelf")
@pytest.mark.parametrize("with_spawn", [False, True])
def test_follow_world_compiles_for_gfx950_without_scratch(with_spawn):
    w = follow_world(with_spawn=with_spawn)
    src = w.generated_kernel_source(compile=True)                          # ggrs_hip_generated_kernel_source(compile=1): builds for gfx950, no device needed
    rtc = C.CDLL("libhiprtc.so")
    prog = C.c_void_p()
    assert rtc.hiprtcCreateProgram(C.byref(prog), src.encode(), b"k.hip", 0, None, None) == 0
    assert rtc.hiprtcCompileProgram(prog, len(OPTS), (C.c_char_p * len(OPTS))(*OPTS)) == 0
    n = C.c_size_t(); rtc.hiprtcGetCodeSize(prog, C.byref(n)); code = C.create_string_buffer(n.value); rtc.hiprtcGetCode(prog, code)
    with tempfile.NamedTemporaryFile(suffix=".hsaco") as f:
        f.write(code.raw); f.flush()
        notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
        asm = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", f.name], capture_output=True, text=True, check=True).stdout
    res = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\d+)", notes)}
    print(res)
    assert res.get("private_segment_fixed_size") == 0 and res.get("vgpr_spill_count") == 0, res
    assert "scratch_" not in asm and "buffer_wbl2" not in asm and "buffer_inv" not in asm       # no scratch access; the kernel boundary is the only synchronisation


def test_worlds_without_peer_bindings_keep_their_text():
    """The headline world's text is the committed golden text (docs/generated/), and a user-written world's text has nothing of the peer view."""
    for form, steady in (("generic", False), ("steady", True)):
        w = bg.World(1_000_000, max_depth=9, flags=bg.GGRS_WORLD_LAYOUT_ONLY); cm.build_particles(w)
        assert w.generated_kernel_source(steady=steady) == open(os.path.join(ROOT, "docs", "generated", f"headline_{form}.hip")).read(), form
    w = layout_world(); A = w.register_component("A", 4, 1); w.checksum_component(A, [0]); w.add_custom_system(NOP, [(A, 0)])
    src = w.generated_kernel_source()
    for ident in NEW_IDENTIFIERS: assert ident not in src, ident
    assert "pv_" not in src and "GgrsPeer" not in src and re.search(r"ggrs_u32 dt_bits\[10\];", src)
