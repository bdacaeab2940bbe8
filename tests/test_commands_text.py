"""Command bindings (ggrs_hip_add_custom_system_commands: a user-written system inserts and removes components of its OWN entity -- e.has / e.opt_* / e.insert /
e.remove), checked WITHOUT a GPU on GGRS_WORLD_LAYOUT_ONLY worlds: the entry point exists in every layer that mirrors the ABI; every rule and refusal of
include/ggrs_hip.h answers GGRS_E_INVALID with a message naming the system, the component or the column; the stun world's generated text rebuilds Stun's mask
word from the lanes and copies Hp's, compiles for gfx950 and needs no scratch; the text of a world without command bindings is what it was; a call to an
undeclared e.insert(j) does not compile."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import bevy_ggrs_amd as bg
import common as cm
from bevy_ggrs_amd import _ffi
from commands_common import BOTH, STUN_SRC, build_shield, build_stun, build_watch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]
NEW_IDENTIFIERS = ("opt_u32", "has_")      # what a world without command bindings does not name
NOP = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) += 1u; }"
OPT = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { if (e.has(0)) e.opt_u32(0, 0) += 1u; }"
INS = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { if (!e.has(0)) { e.opt_u32(0, 0) = e.u32(0); e.insert(0); } }"


def layout_world(cap=600, flags=0):
    return bg.World(cap, max_depth=8, flags=bg.GGRS_WORLD_LAYOUT_ONLY | flags)


def _two(w):
    H = w.register_component("Hp", 4, 1); S = w.register_component("Stun", 4, 2)
    w.checksum_component(H, [0]); w.checksum_component(S, [0, 1])
    return H, S


def _refused(w, *needles):
    with pytest.raises(bg.GgrsHipError) as e:
        w.generated_kernel_source()
    assert e.value.code == bg.GGRS_E_INVALID, str(e.value)
    for n in needles: assert n in str(e.value), (n, str(e.value))


def test_entry_point_exists_in_header_library_ctypes_mirror_and_rust_shim():
    hdr = open(os.path.join(ROOT, "include", "ggrs_hip.h")).read()
    assert re.search(r"int ggrs_hip_add_custom_system_commands\(ggrs_world\* w, const ggrs_custom_system_desc\* desc,\s*const ggrs_peer_binding\* peers, uint32_t n_peers,\s*"
                     r"const ggrs_effect_binding\* effects, uint32_t n_effects,\s*const ggrs_command_binding\* cmds, uint32_t n_cmds\);", hdr)
    assert re.search(r"#define GGRS_CMD_INSERT\s+1u\b", hdr) and re.search(r"#define GGRS_CMD_REMOVE\s+2u\b", hdr)
    assert bg.CMD_INSERT == 1 and bg.CMD_REMOVE == 2
    assert re.search(r"#define GGRS_COMMAND_MAX_BINDINGS\s+4\b", hdr) and re.search(r"#define GGRS_COMMAND_MAX_WORDS\s+8\b", hdr) and "#define GGRS_HIP_ABI_VERSION 9" in hdr
    assert "typedef struct { uint32_t comp; uint32_t flags; } ggrs_command_binding;" in hdr
    assert hasattr(C.CDLL(_ffi.LIB_PATH), "ggrs_hip_add_custom_system_commands") and "ggrs_hip_add_custom_system_commands" in _ffi.SIGNATURES
    assert C.sizeof(_ffi.CommandBinding) == 8 and _ffi.COMMAND_MAX_BINDINGS == 4 and _ffi.COMMAND_MAX_WORDS == 8
    rs = open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "ffi.rs")).read()
    assert ("pub fn ggrs_hip_add_custom_system_commands(w: *mut ggrs_world, desc: *const ggrs_custom_system_desc, peers: *const ggrs_peer_binding, n_peers: u32, "
            "effects: *const ggrs_effect_binding, n_effects: u32, cmds: *const ggrs_command_binding, n_cmds: u32) -> c_int;") in rs
    assert "pub struct ggrs_command_binding {" in rs and "pub const GGRS_CMD_INSERT: u32 = 1;" in rs and "pub const GGRS_CMD_REMOVE: u32 = 2;" in rs
    assert "ggrs_hip_add_custom_system_commands(w, d, peers, n_peers, effects, n_effects, cmds, n_cmds)" in open(os.path.join(ROOT, "include", "bevy_ggrs_hip.hpp")).read()
    for words in ("the last call wins", "insert on a present component replaces its value", "Commands apply even when the same call despawns the entity",
                  "a system registered LATER runs for the entity in the same frame", "a system registered EARLIER sees the change in the next frame",
                  "its own bindings and its command bindings share no component"):
        assert words in hdr, words


def test_zero_commands_is_the_effects_entry_point():
    texts = []
    for how in ("plain", "commands"):
        w = layout_world(); H, S = _two(w)
        if how == "plain": w.add_custom_system(NOP, [(H, 0)])
        else:
            d = _ffi.CustomSystemDesc(); d.name, d.source, d.n_bindings = b"custom", NOP.encode(), 1; d.comp[0], d.word[0] = H, 0
            w._check(w._lib.ggrs_hip_add_custom_system_commands(w._p, C.byref(d), None, 0, None, 0, None, 0))
        texts.append(w.generated_kernel_source())
    assert texts[0] == texts[1] and "GgrsEntityC" not in texts[0] and "opt_u32" not in texts[0] and "has_" not in texts[0]
    assert "const bool p1_0" in texts[0] and "__ballot(p1_0)" not in texts[0]


def test_rule_own_bindings_and_command_bindings_share_no_component():
    w = layout_world(); H, S = _two(w)
    w.add_custom_system(OPT, [(H, 0), (S, 1)], name="stunner", commands=[(S, BOTH)])
    _refused(w, "'stunner'", "'Stun'", "own binding 1", "command binding 0", "share no component")
    w = layout_world(); H, S = _two(w)
    w.add_custom_system(OPT, [(H, 0)], name="stunner", commands=[(S, BOTH), (S, 0)])
    _refused(w, "'stunner'", "'Stun'", "one command binding per system")


def test_rule_a_command_bound_component_counts_as_written_in_every_column():
    # the peer rule: a system with peer bindings is registered before every writer of a column it peer-reads -- word 1 of Stun, which no system names
    reader = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { const GgrsPeer p = e.peer(e.slot); if (p.ok()) e.u32(0) = p.u32(0); }"
    w = layout_world(); H, S = _two(w); B = w.register_component("Beta", 4, 1)
    w.add_custom_system(INS, [(H, 0)], name="stunner", commands=[(S, BOTH)])
    w.add_custom_system(reader, [(B, 0)], name="reader", peers=[(S, 1)])
    _refused(w, "'reader'", "'Stun'", "word 1", "system 0", "writes", "registered before every system that writes a column it peer-reads")
    # ... a flags-0 binding writes too
    w = layout_world(); H, S = _two(w); B = w.register_component("Beta", 4, 1)
    w.add_custom_system(OPT, [(H, 0)], name="toucher", commands=[(S, 0)])
    w.add_custom_system(reader, [(B, 0)], name="reader", peers=[(S, 1)])
    _refused(w, "'reader'", "'Stun'", "word 1", "writes")
    # the other order is accepted
    w = layout_world(); H, S = _two(w); B = w.register_component("Beta", 4, 1)
    w.add_custom_system(reader, [(B, 0)], name="reader", peers=[(S, 1)])
    w.add_custom_system(INS, [(H, 0)], name="stunner", commands=[(S, BOTH)])
    assert "pv_col" in w.generated_kernel_source()
    # the effect rule: no system at or after the first sender binds the column -- a command binding binds every column of its component
    send = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.send_u32(e.slot, 0, 1u); }"
    w = layout_world(); H, S = _two(w)
    w.add_custom_system(send, [(H, 0)], name="striker", effects=[(S, 1, bg.EFFECT_ADD)])
    w.add_custom_system(INS, [(H, 0)], name="stunner", commands=[(S, BOTH)])
    _refused(w, "'striker'", "'Stun'", "word 1", "'stunner'", "no system registered at or after the first sender of a column binds that column")
    # ... the sender's own command binding
    w = layout_world(); H, S = _two(w)
    w.add_custom_system(send, [(H, 0)], name="striker", effects=[(S, 1, bg.EFFECT_ADD)], commands=[(S, 0)])
    _refused(w, "'striker'", "'Stun'", "a sender does not bind a column it sends to")
    # build_layout's write sets: every column of Stun is stored with every steady Save (bit 0 = Hp, bits 1, 2 = Stun)
    w = layout_world(); H, S = _two(w)
    w.add_custom_system(OPT, [(H, 0)], name="toucher", commands=[(S, 0)])
    assert "rows 7 / live" in w.generated_kernel_source(steady=True)


def test_refusals_of_the_first_version():
    # a command-bound component under a Strategy
    w = layout_world(); H, S = _two(w)
    w.register_component_strategy(S, 2, 2, "__device__ void ggrs_store(const GgrsWords& t, GgrsWords& s) { s.u16(0) = (unsigned short)t.u32(0); s.u16(1) = (unsigned short)t.u32(1); }\n"
                                           "__device__ void ggrs_load(const GgrsWords& s, GgrsWords& t) { t.u32(0) = s.u16(0); t.u32(1) = s.u16(1); }")
    w.add_custom_system(INS, [(H, 0)], name="stunner", commands=[(S, BOTH)])
    _refused(w, "'stunner'", "'Stun'", "Strategy")
    # ... registered GGRS_COMP_NO_ROLLBACK
    w = layout_world(); H, S = _two(w); N = w.register_component("Mesh", 4, 1, rollback=False)
    w.add_custom_system(INS, [(H, 0)], name="stunner", commands=[(N, BOTH)])
    _refused(w, "'stunner'", "'Mesh'", "GGRS_COMP_NO_ROLLBACK")
    # a world that keeps RollbackDespawned markers
    w = layout_world(); H, S = _two(w); F = w.register_component("Fuse", 4, 1)
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(F,), word=(0,), iparam=(1, bg.DESPAWN_ROLLBACK))
    w.add_custom_system(INS, [(H, 0)], name="stunner", commands=[(S, BOTH)])
    _refused(w, "command bindings", "RollbackDespawned markers")
    # a world that spawns on the device with e.spawn(n)
    w = layout_world(); H, S = _two(w)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.insert(0); e.spawn(1); }", [(H, 0)], name="stunner", commands=[(S, BOTH)])
    w.add_spawn_system("__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64 k, const GgrsFrame&, const unsigned char*) { e.u32(0) = (ggrs_u32)k; }", bundle=(H,), bindings=[(H, 0)],
                       payload_stride=0xFFFFFFFF)
    _refused(w, "command bindings", "spawns on the device", "e.spawn(n)")
    # worlds without the generated kernel
    for flags in (bg.GGRS_WORLD_NO_GROUPS, bg.GGRS_WORLD_UNFUSED):
        w = layout_world(flags=flags); H, S = _two(w)
        w.add_custom_system(INS, [(H, 0)], name="stunner", commands=[(S, BOTH)])
        _refused(w, "command bindings need the generated request-group kernel")
    # more than GGRS_COMMAND_MAX_BINDINGS bindings, more than GGRS_COMMAND_MAX_WORDS words, bad arguments
    w = layout_world(); H, S = _two(w)
    more = [w.register_component(f"C{k}", 4, 1) for k in range(5)]
    with pytest.raises(ValueError):
        w.add_custom_system(NOP, [(H, 0)], commands=[(c, 0) for c in more])
    d = _ffi.CustomSystemDesc(); d.name, d.source, d.n_bindings = b"many", NOP.encode(), 1; d.comp[0], d.word[0] = H, 0
    cb = (_ffi.CommandBinding * 5)()
    for j, c in enumerate(more): cb[j].comp, cb[j].flags = c, 0
    with pytest.raises(bg.GgrsHipError) as e:
        w._check(w._lib.ggrs_hip_add_custom_system_commands(w._p, C.byref(d), None, 0, None, 0, cb, 5))
    assert e.value.code == bg.GGRS_E_INVALID and "'many'" in str(e.value) and "GGRS_COMMAND_MAX_BINDINGS" in str(e.value)
    W5 = w.register_component("Wide5", 4, 5); W4 = w.register_component("Wide4", 4, 4)
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_custom_system(NOP, [(H, 0)], name="wide", commands=[(W5, 0), (W4, 0)])
    assert e.value.code == bg.GGRS_E_INVALID and "'wide'" in str(e.value) and "9 words" in str(e.value) and "GGRS_COMMAND_MAX_WORDS" in str(e.value)
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_custom_system(NOP, [(H, 0)], name="bad", commands=[(99, 0)])
    assert e.value.code == bg.GGRS_E_INVALID and "command binding 0" in str(e.value)
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_custom_system(NOP, [(H, 0)], name="bad", commands=[(S, 4)])
    assert e.value.code == bg.GGRS_E_INVALID and "GGRS_CMD_" in str(e.value)


def test_no_generated_kernel_knob_is_refused(monkeypatch):
    monkeypatch.setenv("GGRS_TICK_JIT", "0")
    w = layout_world(); H, S = _two(w)
    w.add_custom_system(INS, [(H, 0)], name="stunner", commands=[(S, BOTH)])
    _refused(w, "command bindings need the generated request-group kernel", "GGRS_TICK_JIT=0")


def stun_world(cap=600, **kw):
    w = layout_world(cap)
    ids = build_stun(w, **kw)
    return w, ids


def test_stun_world_text_rebuilds_stuns_mask_and_copies_hps():
    w, (H, S) = stun_world()
    src = w.generated_kernel_source()
    body = src.split('extern "C" __global__')[1]
    assert (H, S) == (0, 1)
    # Stun's presence bit is a mutable register, Hp's a constant; a Save stores the ballot for Stun and the source's word for Hp
    assert "    bool p1_0 = (mk1 >> sh) & 1ull;" in body and "    const bool p0_0 = (mk0 >> sh) & 1ull;" in body
    assert body.count("const uint64_t pm1 = __ballot(p1_0);") == 2 and "pm0" not in body          # (the Saves' store, the live block's)
    assert re.search(r"if \(\(pmask_s >> 1u\) & 1u\) \*reinterpret_cast<uint64_t\*>\(dst \+ \d+ull \+ wi8\) = pm1;", body)
    assert re.search(r"if \(\(pmask_s >> 0u\) & 1u\) \*reinterpret_cast<uint64_t\*>\(dst \+ \d+ull \+ wi8\) = mk0;", body)
    # the opt words: from the registers where the lane has Stun, from the literals of the registered default {9, 77} where it has not
    assert "ent.opt[0] = p1_0 ? (ggrs_u64)w1_0 : 0x9ull;" in body and "ent.opt[1] = p1_0 ? (ggrs_u64)w2_0 : 0x4dull;" in body
    assert "if (p1_0) ent.has_ |= 1u;" in body and "p1_0 = (ent.has_ >> 0u) & 1u;" in body
    assert "if (p1_0) { w1_0 = (uint32_t)(uint32_t)ent.opt[0]; w2_0 = (uint32_t)(uint32_t)ent.opt[1]; }" in body
    # the checksum of Stun is gated by the lane's CURRENT presence bit
    assert "(alive_0 && p1_0) ? " in body
    # the entity is the template, instantiated with what the system declared: INSERT | REMOVE on binding 0, its words from opt[0]
    assert "template <unsigned GGRS_IM, unsigned GGRS_RM, unsigned GGRS_CB> struct GgrsEntityC {" in src
    assert "namespace ggrs_sys_0 {\ntypedef ::GgrsEntityC<0x1u, 0x1u, 0x0u> GgrsEntity;\n#line 1" in src
    # no new launch, no wait, no atomics beyond the checksum folds every world has
    assert body.count("atomicXor") == 2 and "s_sleep" not in body
    # the shield world: the flags-0 binding keeps the bit it was handed, the 8-byte word is not narrowed
    w = layout_world(); build_shield(w)
    sb = w.generated_kernel_source().split('extern "C" __global__')[1]
    assert sb.count("p1_0 = (ent.has_ >> 0u) & 1u;") == 1                                            # the granter; not absorb
    assert "if (p1_0) { w1_0 = (uint64_t)(uint64_t)ent.opt[0]; }" in sb and sb.count("ent.opt[0] = p1_0 ? (ggrs_u64)w1_0 : 0xabcd00000000ull;") == 2
    assert "typedef ::GgrsEntityC<0x0u, 0x0u, 0x0u> GgrsEntity;" in w.generated_kernel_source()     # absorb, drain and tally declared nothing


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")
@pytest.mark.parametrize("which", ["stun", "stun+spawn", "shield", "watch"])
def test_command_worlds_compile_for_gfx950_without_scratch(which):
    w = layout_world()
    if which == "stun": build_stun(w)
    elif which == "stun+spawn": build_stun(w, kills=True, spawn="with")
    elif which == "shield": build_shield(w)
    else: build_watch(w)
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
        res = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\d+)", notes)}
        print(which, "steady" if steady else "generic", res)
        assert res.get("private_segment_fixed_size") == 0 and res.get("vgpr_spill_count") == 0, res
        assert "scratch_" not in asm and res["vgpr_count"] <= 64, res            # every e.opt word is a register; eight waves per SIMD


def test_worlds_without_command_bindings_keep_their_text():
    """The headline world's text is the committed golden text (docs/generated/); the strike world's and the follow world's have nothing of the template."""
    for form, steady in (("generic", False), ("steady", True)):
        w = bg.World(1_000_000, max_depth=9, flags=bg.GGRS_WORLD_LAYOUT_ONLY); cm.build_particles(w)
        assert w.generated_kernel_source(steady=steady) == open(os.path.join(ROOT, "docs", "generated", f"headline_{form}.hip")).read(), form
    from peer_effects_common import build_strike
    from peer_reads_common import build_follow
    for build in (build_strike, build_follow):
        w = layout_world(); build(w)
        src = w.generated_kernel_source()
        assert "struct GgrsEntity {" in src and "GgrsEntityC" not in src and "ggrs_sys_0::GgrsEntity" not in src
        for ident in NEW_IDENTIFIERS: assert ident not in src, ident
    assert getattr(w._lib, "ggrs_hip_add_custom_system_commands")          # (on the parent the symbol is missing: this test fails there too)


def test_an_undeclared_insert_or_remove_does_not_compile():
    for flags, call, flag_name in ((bg.CMD_REMOVE, "insert", "GGRS_CMD_INSERT"), (bg.CMD_INSERT, "remove", "GGRS_CMD_REMOVE"), (0, "insert", "GGRS_CMD_INSERT")):
        w = layout_world(); H, S = _two(w)
        with pytest.raises(bg.GgrsHipError) as e:
            w.add_custom_system(STUN_SRC, [(H, 0)], name="stun", commands=[(S, flags)])
        msg = str(e.value)
        assert e.value.code == bg.GGRS_E_INVALID and "custom system 'stun' does not compile" in msg, msg
        assert f"no matching member function for call to '{call}'" in msg and f"must be declared with {flag_name}" in msg, msg     # the compiler's log
    # the declared flags compile; a binding index that is not a constant does not
    w = layout_world(); H, S = _two(w)
    w.add_custom_system(STUN_SRC, [(H, 0)], name="stun", commands=[(S, BOTH)])
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) { e.insert(f.frame & 1); }", [(H, 0)], name="dyn", commands=[(S, BOTH)])
    assert "no matching member function for call to 'insert'" in str(e.value)
