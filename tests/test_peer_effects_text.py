"""Effect bindings (ggrs_hip_add_custom_system_effects: a user-written system WRITES other entities through e.send_*(slot, j, v)), checked WITHOUT a GPU on
GGRS_WORLD_LAYOUT_ONLY worlds: the entry point exists in every layer that mirrors the ABI; every rule and refusal of include/ggrs_hip.h answers GGRS_E_INVALID
with a message naming the system and the column; the strike world's generated text holds the sends, compiles for gfx950 into native no-return atomics and needs no
scratch; the text of a world without effect bindings is what it was."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import bevy_ggrs_amd as bg
import common as cm
from bevy_ggrs_amd import _ffi
from peer_effects_common import build_strike

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]
NEW_IDENTIFIERS = ("fx_", "GgrsFxView", "send_u32")      # what a world without effect bindings does not name
NOP = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) += 1u; }"
SEND = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.send_u32(e.u64(0), 0, 1u); }"
ADD = bg.EFFECT_ADD


def layout_world(cap=600, flags=0):
    return bg.World(cap, max_depth=8, flags=bg.GGRS_WORLD_LAYOUT_ONLY | flags)


def _two(w):
    L = w.register_component("Link", 8, 1); H = w.register_component("Health", 4, 1)
    w.checksum_component(H, [0])
    return L, H


def _refused(w, *needles):
    with pytest.raises(bg.GgrsHipError) as e:
        w.generated_kernel_source()
    assert e.value.code == bg.GGRS_E_INVALID, str(e.value)
    for n in needles: assert n in str(e.value), (n, str(e.value))


def test_entry_point_exists_in_header_library_ctypes_and_rust_shim():
    hdr = open(os.path.join(ROOT, "include", "ggrs_hip.h")).read()
    assert re.search(r"int ggrs_hip_add_custom_system_effects\(ggrs_world\* w, const ggrs_custom_system_desc\* desc,\s*const ggrs_peer_binding\* peers, uint32_t n_peers,\s*"
                     r"const ggrs_effect_binding\* effects, uint32_t n_effects\);", hdr)
    for k, name in enumerate(("ADD", "MIN_U", "MAX_U", "MIN_I", "MAX_I", "OR", "AND", "XOR")):
        assert re.search(r"#define GGRS_EFFECT_%s\s+%du\b" % (name, k), hdr), name
        assert getattr(bg, "EFFECT_" + name) == k
    assert re.search(r"#define GGRS_EFFECT_MAX_BINDINGS\s+8\b", hdr) and re.search(r"#define GGRS_EFFECT_MAX_COLUMNS\s+8\b", hdr) and "#define GGRS_HIP_ABI_VERSION 9" in hdr
    assert "typedef struct { uint32_t comp; uint32_t word; uint32_t op; } ggrs_effect_binding;" in hdr
    assert hasattr(C.CDLL(_ffi.LIB_PATH), "ggrs_hip_add_custom_system_effects") and "ggrs_hip_add_custom_system_effects" in _ffi.SIGNATURES
    assert C.sizeof(_ffi.EffectBinding) == 12
    rs = open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "ffi.rs")).read()
    assert ("pub fn ggrs_hip_add_custom_system_effects(w: *mut ggrs_world, desc: *const ggrs_custom_system_desc, peers: *const ggrs_peer_binding, n_peers: u32, "
            "effects: *const ggrs_effect_binding, n_effects: u32) -> c_int;") in rs
    assert "ffi::ggrs_hip_add_custom_system_effects(" in open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "lib.rs")).read()
    assert "ggrs_hip_add_custom_system_effects(w, d, peers, n_peers, effects, n_effects)" in open(os.path.join(ROOT, "include", "bevy_ggrs_hip.hpp")).read()
    # the semantics, in the header's words
    for words in ("All sends of a frame land after the frame's systems and host-decided spawns, and before anything observes the frame",
                  "Entities spawned in this frame cannot be hit.", "A target despawned in this frame drops the send.",
                  "A sender that calls e.despawn() in the same call still sends.", "commutative and", "A float add has neither property and is refused"):
        assert words in hdr, words


def test_zero_effects_is_the_peers_entry_point():
    texts = []
    for how in ("plain", "effects"):
        w = layout_world(); L, H = _two(w)
        if how == "plain": w.add_custom_system(NOP, [(H, 0)])
        else:
            d = _ffi.CustomSystemDesc(); d.name, d.source, d.n_bindings = b"custom", NOP.encode(), 1; d.comp[0], d.word[0] = H, 0
            w._check(w._lib.ggrs_hip_add_custom_system_effects(w._p, C.byref(d), None, 0, None, 0))
        texts.append(w.generated_kernel_source())
    assert texts[0] == texts[1] and "fx_" not in texts[0] and "GgrsFxView" not in texts[0]


def test_rule_no_system_at_or_after_the_first_sender_binds_the_column():
    # a custom system registered after the sender binds the column
    w = layout_world(); L, H = _two(w)
    w.add_custom_system(SEND, [(L, 0)], name="striker", effects=[(H, 0, ADD)])
    w.add_custom_system(NOP, [(H, 0)], name="healer")
    _refused(w, "'striker'", "'Health'", "word 0", "'healer'", "no system registered at or after the first sender of a column binds that column")
    # a built-in system registered after it
    w = layout_world(); L, H = _two(w)
    w.add_custom_system(SEND, [(L, 0)], name="striker", effects=[(H, 0, ADD)])
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, 0))
    _refused(w, "'striker'", "'Health'", "built-in", "binds")
    # (a peer binding of a later system: the peer rules answer first -- the next test)
    # the sender itself
    w = layout_world(); L, H = _two(w)
    w.add_custom_system(SEND, [(L, 0), (H, 0)], name="striker", effects=[(H, 0, ADD)])
    _refused(w, "'striker'", "'Health'", "a sender does not bind a column it sends to")
    # a death system registered BEFORE the sender is accepted: it sees the damage at the start of the next frame
    w = layout_world(); L, H = _two(w)
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, 0))
    w.add_custom_system(SEND, [(L, 0)], name="striker", effects=[(H, 0, ADD)])
    assert "a.fx_col[0]" in w.generated_kernel_source()


def test_rule_a_sender_counts_as_a_writer_for_the_peer_rules():
    w = layout_world(); L, H = _two(w); B = w.register_component("Beta", 4, 1)
    w.add_custom_system(SEND, [(L, 0)], name="striker", effects=[(H, 0, ADD)])
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { const GgrsPeer p = e.peer(e.u64(1)); if (p.ok()) e.u32(0) = p.u32(0); }",
                        [(B, 0), (L, 0)], name="reader", peers=[(H, 0)])
    _refused(w, "'reader'", "'Health'", "system 0", "writes", "registered before every system that writes a column it peer-reads")


def test_rule_one_op_per_column_and_the_component_kind():
    # two ops on one column
    w = layout_world(); L, H = _two(w)
    w.add_custom_system(SEND, [(L, 0)], name="striker", effects=[(H, 0, ADD)])
    w.add_custom_system(SEND, [(L, 0)], name="marker", effects=[(H, 0, bg.EFFECT_OR)])
    _refused(w, "'marker'", "'Health'", "GGRS_EFFECT_OR", "GGRS_EFFECT_ADD", "a column has one op in the whole world")
    # a component under a Strategy
    w = layout_world(); L, H = _two(w)
    w.register_component_strategy(H, 2, 1, "__device__ void ggrs_store(const GgrsWords& t, GgrsWords& s) { s.u16(0) = (unsigned short)t.u32(0); }\n"
                                           "__device__ void ggrs_load(const GgrsWords& s, GgrsWords& t) { t.u32(0) = s.u16(0); }")
    w.add_custom_system(SEND, [(L, 0)], name="striker", effects=[(H, 0, ADD)])
    _refused(w, "'striker'", "'Health'", "Strategy")
    # a non-rollback component
    w = layout_world(); L, H = _two(w); N = w.register_component("Mesh", 4, 1, rollback=False)
    w.add_custom_system(SEND, [(L, 0)], name="striker", effects=[(N, 0, ADD)])
    _refused(w, "'striker'", "'Mesh'", "GGRS_COMP_NO_ROLLBACK")
    # 2-byte words
    w = layout_world(); L, H = _two(w); N = w.register_component("Small", 2, 1)
    w.add_custom_system(SEND, [(L, 0)], name="striker", effects=[(N, 0, ADD)])
    _refused(w, "'striker'", "'Small'", "4- or 8-byte words")


def test_refusals_of_the_first_version():
    # a world that keeps RollbackDespawned markers
    w = layout_world(); L, H = _two(w); F = w.register_component("Fuse", 4, 1)
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(F,), word=(0,), iparam=(1, bg.DESPAWN_ROLLBACK))
    w.add_custom_system(SEND, [(L, 0)], name="striker", effects=[(H, 0, ADD)])
    _refused(w, "effect bindings", "RollbackDespawned markers")
    # a world that spawns on the device with e.spawn(n)
    w = layout_world(); L, H = _two(w)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.send_u32(e.u64(0), 0, 1u); e.spawn(1); }", [(L, 0)], name="striker", effects=[(H, 0, ADD)])
    w.add_spawn_system("__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64 k, const GgrsFrame&, const unsigned char*) { e.u64(0) = k; }", bundle=(L,), bindings=[(L, 0)],
                       payload_stride=0xFFFFFFFF)
    _refused(w, "effect bindings", "spawns on the device", "e.spawn(n)")
    # worlds without the generated kernel
    for flags in (bg.GGRS_WORLD_NO_GROUPS, bg.GGRS_WORLD_UNFUSED):
        w = layout_world(flags=flags); L, H = _two(w)
        w.add_custom_system(SEND, [(L, 0)], name="striker", effects=[(H, 0, ADD)])
        _refused(w, "effect bindings need the generated request-group kernel")
    # more than GGRS_EFFECT_MAX_COLUMNS distinct effect columns
    w = layout_world(); L, H = _two(w); W = w.register_component("Wide", 4, 9)
    w.add_custom_system(SEND, [(L, 0)], name="a", effects=[(W, k, ADD) for k in range(8)])
    w.add_custom_system(SEND, [(L, 0)], name="b", effects=[(W, 8, ADD)])
    _refused(w, "9 distinct effect columns", "GGRS_EFFECT_MAX_COLUMNS")
    # bad arguments
    w = layout_world(); L, H = _two(w)
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_custom_system(SEND, [(L, 0)], effects=[(7, 0, ADD)])
    assert e.value.code == bg.GGRS_E_INVALID and "effect binding 0" in str(e.value)
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_custom_system(SEND, [(L, 0)], effects=[(H, 0, 8)])
    assert e.value.code == bg.GGRS_E_INVALID and "GGRS_EFFECT_" in str(e.value)
    with pytest.raises(ValueError):
        w.add_custom_system(SEND, [(L, 0)], effects=[(H, 0, ADD)] * 9)


def test_no_generated_kernel_knob_is_refused(monkeypatch):
    monkeypatch.setenv("GGRS_TICK_JIT", "0")
    w = layout_world(); L, H = _two(w)
    w.add_custom_system(SEND, [(L, 0)], name="striker", effects=[(H, 0, ADD)])
    _refused(w, "effect bindings need the generated request-group kernel", "GGRS_TICK_JIT=0")


def strike_world(cap=600, **kw):
    w = layout_world(cap)
    build_strike(w, **kw)
    return w


def test_strike_world_text_holds_the_sends_and_groups_that_end_on_their_step():
    src = strike_world().generated_kernel_source()
    body = src.split('extern "C" __global__')[1]
    # the inbox's base pointers and the bounds length are in the argument block, the four effect columns only; no peer view in this world
    assert re.search(r"unsigned char\* fx_col\[4\];", src) and "ggrs_u64 fx_len;" in src and "pv_col" not in src
    # e.send_*: a bounds test against the source block's len, then one relaxed agent-scope atomic whose result is unused
    assert "if (s >= fx_.len || fx_.wb[j] != 4) return;" in src and "if (s >= fx_.len || fx_.wb[j] != 8) return;" in src
    for op in ("add", "min", "max", "or", "and", "xor"):
        assert f"(void)__hip_atomic_fetch_{op}(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);" in src, op
    assert "ent.fx_.len = a.fx_len;" in body
    for j, (wb, op) in enumerate(((4, bg.EFFECT_ADD), (4, bg.EFFECT_OR), (4, bg.EFFECT_MIN_I), (8, bg.EFFECT_ADD))):
        assert f"ent.fx_.col[{j}] = (unsigned long)a.fx_col[{j}]; ent.fx_.wb[{j}] = {wb}u; ent.fx_.op[{j}] = {op}u;" in body, j
    # one AdvanceWorld per launch: every per-step array of the argument block has one element
    assert re.search(r"ggrs_u32 dt_bits\[1\];", src) and re.search(r"int step_frame\[1\];", src)
    # a specialised copy keeps the inbox's pointers as arguments
    steady = strike_world().generated_kernel_source(steady=True)
    assert "a.fx_len" in steady and "a.fx_col[3]" in steady
    # peer reads and effects in ONE system: both the view and the inbox
    both = strike_world(order="first").generated_kernel_source()
    assert re.search(r"const unsigned char\* pv_col\[1\];", both) and re.search(r"unsigned char\* fx_col\[4\];", both)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")
@pytest.mark.parametrize("order,with_spawn", [("last", False), ("first", True)])
def test_strike_world_compiles_to_native_no_return_atomics_without_scratch(order, with_spawn):
    w = strike_world(order=order, with_spawn=with_spawn)
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
    atomics = [ln.split("//")[0].split() for ln in asm.splitlines() if "global_atomic_" in ln]
    print(res, [a[0] for a in atomics])
    # Hp ADD, Flags OR, Low MIN_I (signed), Score ADD on 8 bytes: one native instruction each, no compare-and-swap loop, no returned value (no sc0)
    assert sorted(a[0] for a in atomics) == ["global_atomic_add", "global_atomic_add_x2", "global_atomic_or", "global_atomic_smin"], atomics
    assert "cmpswap" not in asm and not any("sc0" in a for a in atomics), atomics
    assert res.get("private_segment_fixed_size") == 0 and res.get("vgpr_spill_count") == 0, res
    assert "scratch_" not in asm and "buffer_wbl2" not in asm and "buffer_inv" not in asm       # no scratch access; the kernel boundary is the only synchronisation


def test_worlds_without_effect_bindings_keep_their_text():
    """The headline world's text is the committed golden text (docs/generated/); a user-written world's and a peer world's text have nothing of the inbox."""
    for form, steady in (("generic", False), ("steady", True)):
        w = bg.World(1_000_000, max_depth=9, flags=bg.GGRS_WORLD_LAYOUT_ONLY); cm.build_particles(w)
        assert w.generated_kernel_source(steady=steady) == open(os.path.join(ROOT, "docs", "generated", f"headline_{form}.hip")).read(), form
    w = layout_world(); A = w.register_component("A", 4, 1); w.checksum_component(A, [0]); w.add_custom_system(NOP, [(A, 0)])
    src = w.generated_kernel_source()
    for ident in NEW_IDENTIFIERS: assert ident not in src, ident
    assert re.search(r"ggrs_u32 dt_bits\[10\];", src)
    from peer_reads_common import build_follow
    w = layout_world(); build_follow(w)
    src = w.generated_kernel_source()
    assert "GgrsPeer" in src
    for ident in NEW_IDENTIFIERS: assert ident not in src, ident
    assert getattr(w._lib, "ggrs_hip_add_custom_system_effects")          # (on the parent the symbol is missing: this test fails there too)
