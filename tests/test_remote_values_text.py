"""Remote inserts that carry the sender's value (ggrs_hip_add_custom_system_values: e.val_*(j, k) / e.send_value(slot, j); the last sender in schedule order wins, as
one value), checked WITHOUT a GPU on GGRS_WORLD_LAYOUT_ONLY worlds: the entry point exists in every layer that mirrors the ABI; every refusal answers
GGRS_E_INVALID with a message naming the system and the component; an undeclared j, an accessor of the other width, a k out of range or a j / k that is no constant
does not compile; the new text appears only in worlds with a value binding -- the hit world of the remote-command tests keeps the parent's text byte for byte
(tests/golden/) --; the brand world's kernels compile for gfx950 without scratch, the key sent with a native 64-bit atomic max; and the ORACLE sessions the GPU tests
compare against reach every conflict the contract names (the coverage floors)."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

import pytest

import bevy_ggrs_amd as bg
import common as cm
from bevy_ggrs_amd import _ffi
from oracle.binding import FLAT, OracleWorld
from remote_commands_common import build_hit
from remote_values_common import (Stats, all_to_zero_links, build_brand, p2p_lists, run_oracle, spawn_brand, spawn_patch, synctest_lists)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]
NEW_IDENTIFIERS = ("rv_win", "rv_pay", "send_value", "val_u32", "GGRS_XV", "GGRS_VB", "vw_", "vt_", "__hip_atomic_fetch_max")     # what a world without value bindings does not name
NOP = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) += 1u; }"
BRAND = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.val_u32(0, 0) = 4u; e.val_u32(0, 1) = (ggrs_u32)e.slot; e.send_value(e.u64(0), 0); }"
KILL = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.send_despawn(e.u64(0)); }"
INS, REM, DSP, ENT = bg.REMOTE_INSERT, bg.REMOTE_REMOVE, bg.REMOTE_DESPAWN, bg.REMOTE_ENTITY


def layout_world(cap=600, flags=0):
    return bg.World(cap, max_depth=8, flags=bg.GGRS_WORLD_LAYOUT_ONLY | flags)


def _three(w):
    H = w.register_component("Hp", 4, 1); T = w.register_component("Target", 8, 1); S = w.register_component("Stun", 4, 2)
    for c, words in ((H, [0]), (T, [0]), (S, [0, 1])): w.checksum_component(c, words)
    return H, T, S


def _refused(w, *needles):
    with pytest.raises(bg.GgrsHipError) as e:
        w.generated_kernel_source()
    assert e.value.code == bg.GGRS_E_INVALID, str(e.value)
    for n in needles: assert n in str(e.value), (n, str(e.value))


def test_entry_point_exists_in_header_library_ctypes_mirror_cpp_backend_and_rust_shim():
    hdr = open(os.path.join(ROOT, "include", "ggrs_hip.h")).read()
    assert re.search(r"int ggrs_hip_add_custom_system_values\(ggrs_world\* w, const ggrs_custom_system_desc\* desc,\s*const ggrs_peer_binding\* peers, uint32_t n_peers,\s*"
                     r"const ggrs_effect_binding\* effects, uint32_t n_effects,\s*const ggrs_command_binding\* cmds, uint32_t n_cmds,\s*const ggrs_resource_binding\* res, uint32_t n_res,\s*"
                     r"const ggrs_reduce_binding\* red, uint32_t n_red,\s*const ggrs_remote_binding\* rem, uint32_t n_rem,\s*const ggrs_sum_binding\* sum, uint32_t n_sum,\s*"
                     r"const ggrs_value_binding\* val, uint32_t n_val\);", hdr)
    assert "typedef struct { uint32_t comp; uint32_t flags; } ggrs_value_binding;" in hdr and "#define GGRS_HIP_ABI_VERSION 9" in hdr
    for name, val in (("GGRS_VALUE_MAX_BINDINGS", "4"), ("GGRS_VALUE_MAX_WORDS", "8"), ("GGRS_VALUE_MAX_WORLD_BINDINGS", "16")):
        assert re.search(rf"#define {name}\s+{val}\b", hdr), name
    assert (bg.VALUE_MAX_BINDINGS, bg.VALUE_MAX_WORDS, bg.VALUE_MAX_WORLD_BINDINGS) == (4, 8, 16)
    lib = C.CDLL(_ffi.LIB_PATH)
    assert hasattr(lib, "ggrs_hip_add_custom_system_values") and "ggrs_hip_add_custom_system_values" in _ffi.SIGNATURES and hasattr(lib, "ggrs_dbg_value_winners")
    assert C.sizeof(_ffi.ValueBinding) == 8
    rs = open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "ffi.rs")).read()
    assert "pub fn ggrs_hip_add_custom_system_values(w: *mut ggrs_world, " in rs and "val: *const ggrs_value_binding, n_val: u32) -> c_int;" in rs
    assert "pub struct ggrs_value_binding {" in rs and "pub const GGRS_VALUE_MAX_WORLD_BINDINGS: usize = 16;" in rs
    assert ("ggrs_hip_add_custom_system_values(w, d, peers, n_peers, effects, n_effects, cmds, n_cmds, res, n_res, red, n_red, rem, n_rem, sum, n_sum, val, n_val)"
            in open(os.path.join(ROOT, "include", "bevy_ggrs_hip.hpp")).read())
    # the header states the contract: the conflict rules, the key, "one command per binding and call", and that the words arrive together
    for words in ("DESPAWN WINS OVER EVERYTHING", "REMOVE WINS OVER ANY INSERT", "A VALUE WINS OVER A DEFAULT INSERT", "AMONG VALUES THE LARGEST KEY WINS", "key = (g + 1) << 40 | (sender slot + 1)",
                  "ONE COMMAND PER BINDING AND CALL", "THE WINNER'S WORDS ARRIVE TOGETHER", "declares several value bindings of the same component", "AS THEY STAND WHEN ggrs_system RETURNS"):
        assert words in hdr, words


def test_zero_value_bindings_is_the_sums_entry_point():
    texts = []
    for how in ("sums", "values"):
        w = layout_world(); H, T, S = _three(w)
        d = _ffi.CustomSystemDesc(); d.name, d.source, d.n_bindings = b"custom", NOP.encode(), 1; d.comp[0], d.word[0] = H, 0
        if how == "sums": w._check(w._lib.ggrs_hip_add_custom_system_sums(w._p, C.byref(d), None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0))
        else: w._check(w._lib.ggrs_hip_add_custom_system_values(w._p, C.byref(d), None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0))
        texts.append(w.generated_kernel_source())
    w = layout_world(); H, T, S = _three(w); w.add_custom_system(NOP, [(H, 0)], values=[])           # the Python mirror: an empty list goes through the new entry point
    texts.append(w.generated_kernel_source())
    assert texts[0] == texts[1] == texts[2]
    for ident in NEW_IDENTIFIERS + ("GgrsEntityC", "rx_inbox"): assert ident not in texts[0], ident


def test_a_value_bound_component_is_a_remotely_commanded_component_in_every_rule():
    # the binding order: a reader registered after the first value sender
    w = layout_world(); H, T, S = _three(w)
    w.add_custom_system(BRAND, [(T, 0)], name="brander", values=[S])
    w.add_custom_system(NOP, [(S, 1)], name="reader")
    _refused(w, "'brander'", "'Stun'", "'reader'", "no system registered at or after the first remote commander of a component binds that component")
    # the sender itself
    w = layout_world(); H, T, S = _three(w)
    w.add_custom_system(BRAND, [(T, 0), (S, 0)], name="brander", values=[S])
    _refused(w, "'brander'", "'Stun'", "a remote commander does not bind a component it commands")
    # a system registered BEFORE may bind it
    w = layout_world(); H, T, S = _three(w)
    w.add_custom_system(NOP, [(S, 1)], name="reader")
    w.add_custom_system(BRAND, [(T, 0)], name="brander", values=[S])
    assert "rv_win" in w.generated_kernel_source()
    # after a remote despawner
    w = layout_world(); H, T, S = _three(w)
    w.add_custom_system(KILL, [(T, 0)], name="killer", remote=[(ENT, DSP)])
    w.add_custom_system(BRAND, [(T, 0)], name="brander", values=[S])
    _refused(w, "'brander'", "'killer'", "has value bindings", "no system registered after a remote despawner")
    # under a Strategy
    w = layout_world(); H, T, S = _three(w)
    w.register_component_strategy(S, 2, 2, "__device__ void ggrs_store(const GgrsWords& t, GgrsWords& s) { s.u16(0) = (unsigned short)t.u32(0); s.u16(1) = (unsigned short)t.u32(1); }\n"
                                           "__device__ void ggrs_load(const GgrsWords& s, GgrsWords& t) { t.u32(0) = s.u16(0); t.u32(1) = s.u16(1); }")
    w.add_custom_system(BRAND, [(T, 0)], name="brander", values=[S])
    _refused(w, "'brander'", "value binding 0", "'Stun'", "Strategy")
    # not rollback
    w = layout_world(); H, T, S = _three(w); N = w.register_component("Mesh", 4, 2, rollback=False)
    w.add_custom_system(BRAND, [(T, 0)], name="brander", values=[N])
    _refused(w, "'brander'", "value binding 0", "'Mesh'", "GGRS_COMP_NO_ROLLBACK")
    # an effect column of the same world
    w = layout_world(); H, T, S = _three(w)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.send_u32(e.u64(0), 0, 1u); e.val_u32(0, 0) = 1u; e.send_value(e.u64(0), 0); }", [(T, 0)], name="brander",
                        effects=[(S, 1, bg.EFFECT_ADD)], values=[S])
    _refused(w, "'brander'", "value binding 0", "'Stun'", "effect column", "not supported in this version")
    # GGRS_REMOTE_MAX_COMPONENTS counts both kinds together: 4 remote + 4 value + 1 value
    w = layout_world(); H, T, S = _three(w)
    more = [w.register_component(f"C{k}", 4, 1) for k in range(9)]
    w.add_custom_system(NOP, [(H, 0)], name="s0", remote=[(c, INS) for c in more[:4]])
    w.add_custom_system(NOP, [(H, 0)], name="s1", values=more[4:8])
    w.add_custom_system(NOP, [(H, 0)], name="s2", values=more[8:9])
    _refused(w, "9 distinct remotely commanded components", "GGRS_REMOTE_MAX_COMPONENTS")


def test_world_refusals_stay(monkeypatch):
    # a world that keeps RollbackDespawned markers
    w = layout_world(); H, T, S = _three(w); F = w.register_component("Fuse", 4, 1)
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(F,), word=(0,), iparam=(1, bg.DESPAWN_ROLLBACK))
    w.add_custom_system(BRAND, [(T, 0)], name="brander", values=[S])
    _refused(w, "RollbackDespawned markers")
    # a world that spawns on the device with e.spawn(n)
    w = layout_world(); H, T, S = _three(w)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.val_u32(0, 0) = 1u; e.send_value(e.u64(0), 0); e.spawn(1); }", [(T, 0)], name="brander", values=[S])
    w.add_spawn_system("__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64 k, const GgrsFrame&, const unsigned char*) { e.u32(0) = (ggrs_u32)k; }", bundle=(H,), bindings=[(H, 0)],
                       payload_stride=0xFFFFFFFF)
    _refused(w, "spawns on the device", "e.spawn(n)")
    # worlds without the generated kernel
    for flags in (bg.GGRS_WORLD_NO_GROUPS, bg.GGRS_WORLD_UNFUSED):
        w = layout_world(flags=flags); H, T, S = _three(w)
        w.add_custom_system(BRAND, [(T, 0)], name="brander", values=[S])
        _refused(w, "need the generated request-group kernel")
    monkeypatch.setenv("GGRS_TICK_JIT", "0")
    w = layout_world(); H, T, S = _three(w)
    w.add_custom_system(BRAND, [(T, 0)], name="brander", values=[S])
    _refused(w, "need the generated request-group kernel", "GGRS_TICK_JIT=0")


def test_limits_flags_and_word_sizes():
    # more than GGRS_VALUE_MAX_BINDINGS per system
    w = layout_world(); H, T, S = _three(w)
    with pytest.raises(ValueError):
        w.add_custom_system(NOP, [(H, 0)], values=[H] * 5)
    d = _ffi.CustomSystemDesc(); d.name, d.source, d.n_bindings = b"many", NOP.encode(), 1; d.comp[0], d.word[0] = H, 0
    vb = (_ffi.ValueBinding * 5)()
    for j in range(5): vb[j].comp, vb[j].flags = H, 0
    with pytest.raises(bg.GgrsHipError) as e:
        w._check(w._lib.ggrs_hip_add_custom_system_values(w._p, C.byref(d), None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, vb, 5))
    assert e.value.code == bg.GGRS_E_INVALID and "'many'" in str(e.value) and "GGRS_VALUE_MAX_BINDINGS" in str(e.value)
    # more than GGRS_VALUE_MAX_WORDS staged words per system: 3 x 3
    w = layout_world(); H, T, S = _three(w); B = w.register_component("Burn", 4, 3)
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_custom_system(NOP, [(H, 0)], name="wide", values=[B, B, B])
    assert e.value.code == bg.GGRS_E_INVALID and "'wide'" in str(e.value) and "9 words" in str(e.value) and "GGRS_VALUE_MAX_WORDS" in str(e.value)
    # flags != 0, an unknown component
    for val, needles in (([(S, 8)], ("'bad'", "'Stun'", "flags must be 0")), ([(S, 1)], ("'bad'", "'Stun'", "flags must be 0")), ([99], ("'bad'", "value binding 0", "not registered"))):
        with pytest.raises(bg.GgrsHipError) as e:
            w.add_custom_system(NOP, [(H, 0)], name="bad", values=val)
        assert e.value.code == bg.GGRS_E_INVALID, str(e.value)
        for n in needles: assert n in str(e.value), (n, str(e.value))
    # ggrs_remote_binding is unchanged: flag value 8 on a REMOTE binding is still refused
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_custom_system(NOP, [(H, 0)], name="bad", remote=[(S, 8)])
    assert "GGRS_REMOTE_" in str(e.value)
    # words of 4 or 8 bytes only
    w = layout_world(); H, T, S = _three(w); N = w.register_component("Narrow", 2, 2)
    w.add_custom_system(NOP, [(H, 0)], name="brander", values=[N])
    _refused(w, "'brander'", "value binding 0", "'Narrow'", "2 bytes", "4 or 8 bytes")
    # more than GGRS_VALUE_MAX_WORLD_BINDINGS per world: 5 systems x 4 bindings of one component
    w = layout_world(); H, T, S = _three(w)
    for k in range(5): w.add_custom_system(NOP, [(H, 0)], name=f"s{k}", values=[S, S, S, S] if k < 4 else [S])
    _refused(w, "17 in this world", "GGRS_VALUE_MAX_WORLD_BINDINGS", "'s4'", "'Stun'")
    # a component bound twice by one system is allowed: that is how a system hits several targets
    w = layout_world(); H, T, S = _three(w)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.val_u32(0, 0) = 1u; e.val_u32(1, 1) = 2u; e.send_value(e.u64(0), 0); e.send_value(e.u64(0) + 1ull, 1); }",
                        [(T, 0)], name="twice", values=[S, S])
    src = w.generated_kernel_source()
    assert "typedef ::GgrsEntityC<0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0u, 0x3u, 0x420u> GgrsEntity;" in src          # bindings 0 and 1 declared, 4-byte words; bases 0, 2, end 4


def test_an_undeclared_wrong_width_out_of_range_or_non_constant_accessor_does_not_compile():
    body = lambda b: "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) { " + b + " }"
    # value bindings 0 = Stun (2 x 4 bytes), 1 = Mark (1 x 8 bytes)
    cases = ((body("e.val_u32(2, 0) = 1u;"), "val_u32"),                      # an undeclared j
             (body("e.send_value(e.u64(0), 2);"), "send_value"),
             (body("e.val_u64(0, 0) = 1ull;"), "val_u64"),                    # the other width: Stun has 4-byte words
             (body("e.val_u32(1, 0) = 1u;"), "val_u32"),                      # ... and Mark 8-byte ones
             (body("e.val_f32(1, 0) = 1.f;"), "val_f32"),
             (body("e.val_u32(0, 2) = 1u;"), "val_u32"),                      # k out of range: Stun has words 0 and 1
             (body("e.val_u64(1, 1) = 1ull;"), "val_u64"),
             (body("e.val_u32(0, f.frame & 1) = 1u;"), "val_u32"),            # k not a constant
             (body("e.val_i32(f.frame & 1, 0) = 1;"), "val_i32"),             # j not a constant
             (body("e.send_value(e.u64(0), f.frame & 1);"), "send_value"))
    for src, call in cases:
        w = layout_world(); H, T, S = _three(w); M = w.register_component("Mark", 8, 1)
        with pytest.raises(bg.GgrsHipError) as e:
            w.add_custom_system(src, [(T, 0)], name="brander", values=[S, M])
        msg = str(e.value)
        assert e.value.code == bg.GGRS_E_INVALID and "custom system 'brander' does not compile" in msg, msg
        assert f"no matching member function for call to '{call}'" in msg, msg                                 # the compiler's log
    # what is declared compiles: every accessor of the right width, every word
    w = layout_world(); H, T, S = _three(w); M = w.register_component("Mark", 8, 1)
    w.add_custom_system(body("e.val_u32(0, 0) = 1u; e.val_i32(0, 1) = -2; e.val_f32(1, 1) = 1.5f; e.val_u64(2, 0) = 1ull << 40; e.send_value(e.u64(0), 0); e.send_value(e.u64(0), 1); e.send_value(e.u64(0), 2);"),
                        [(T, 0)], name="brander", values=[S, S, M])
    assert "0x47u, 0x5420u> GgrsEntity;" in w.generated_kernel_source()         # three bindings, binding 2 is 8 bytes wide; bases 0, 2, 4, end 5
    # a system WITHOUT value bindings has no such member at all
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_custom_system(BRAND, [(T, 0)], name="plain")
    assert "val_u32" in str(e.value) or "send_value" in str(e.value)


def brand_world(cap=600, n=300, **kw):
    w = layout_world(cap)
    return w, build_brand(w, n, **kw)


def test_brand_world_text_stages_defaults_stores_at_the_own_slot_and_sends_one_max_and_one_or():
    w, ids = brand_world()
    src = w.generated_kernel_source()
    body = src.split('extern "C" __global__')[1]
    assert ids == (0, 1, 2, 3, 4)
    # the argument block: Burn and Mark are remotely commanded components 0 and 1; four value bindings in the world
    assert re.search(r"ggrs_u64\* rv_win\[2\];", src) and re.search(r"unsigned char\* rv_pay\[4\];", src) and re.search(r"ggrs_u32\* rx_inbox;", src)
    assert "unsigned GGRS_XD, unsigned GGRS_XV, unsigned GGRS_VB> struct GgrsEntityC {" in src
    assert "namespace ggrs_sys_1 {\ntypedef ::GgrsEntityC<0x0u, 0x0u, 0x0u, 0x1u, 0x1u, 0u, 0x3u, 0x630u> GgrsEntity;\n#line 1" in src      # torch: two Burn bindings, bases 0, 3, end 6
    assert "namespace ggrs_sys_2 {\ntypedef ::GgrsEntityC<0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 1u, 0x13u, 0x410u> GgrsEntity;\n#line 1" in src     # tagger: Mark (8 bytes) at 0, Burn at 1, end 4
    # the staged words start at the default literals: Burn {1.5f, 3, 0xFFFFFFFF} twice in torch; Mark 7 and Burn in the tagger
    assert body.count("ent.vw_[0] = 0x3fc00000ull;") == 1 and body.count("ent.vw_[3] = 0x3fc00000ull;") == 1 and "ent.vw_[5] = 0xffffffffull;" in body
    assert "ent.vw_[0] = 0x7ull;" in body and "ent.vw_[1] = 0x3fc00000ull;" in body
    # per binding: the words at the sender's own slot (word-major, cap_pad entries), ONE atomic max of the key, ONE atomic or of the value bit
    cap_pad = int(re.search(r"a\.rv_pay\[0\] \+ \((\d+)ull \+ e0\) \* 4ull\) = \(ggrs_u32\)ent\.vw_\[1\];", body).group(1))
    assert cap_pad >= 600 and cap_pad % 64 == 0
    assert f"a.rv_pay[1] + ({2 * cap_pad}ull + e0) * 4ull) = (ggrs_u32)ent.vw_[5];" in body
    assert "*(GGRS_G ggrs_u64*)((unsigned long)a.rv_pay[2] + (0ull + e0) * 8ull) = (ggrs_u64)ent.vw_[0];" in body
    assert body.count("__hip_atomic_fetch_max(") == 4
    for g, comp_at, j in ((0, 0, 0), (1, 0, 1), (2, 1, 0), (3, 0, 1)):
        assert (f"__hip_atomic_fetch_max((GGRS_G ggrs_u64*)((unsigned long)a.rv_win[{comp_at}] + (ent.vt_[{j}] << 3)), {hex((g + 1) << 40)}ull | ((ggrs_u64)e0 + 1ull), __ATOMIC_RELAXED, "
                "__HIP_MEMORY_SCOPE_AGENT);") in body, (g, comp_at, j)
    assert body.count("(ent.vt_[0] << 2)), 0x20000u,") == 1 and body.count("(ent.vt_[1] << 2)), 0x20000u,") == 2 and body.count("(ent.vt_[0] << 2)), 0x40000u,") == 1      # bits 17 and 18
    assert body.count("if (ent.vt_[0] < ent.rxn_) {") == 2 and body.count("if (ent.vt_[1] < ent.rxn_) {") == 2
    assert "__syncthreads" not in body.split("ggrs_sys_1::ggrs_system")[1].split("ggrs_sys_2::ggrs_system")[0]
    # a specialised copy keeps the pointers as arguments
    steady = w.generated_kernel_source(steady=True)
    assert "a.rv_win[0]" in steady and "a.rv_pay[3]" in steady and "a.rx_inbox" in steady
    # the effect variant reads fx_len
    w, ids = brand_world(effects=True)
    both = w.generated_kernel_source()
    assert "ent.rxn_ = a.fx_len;" in both and "rx_len" not in both and "a.rv_win[0]" in both


def test_worlds_without_value_bindings_keep_their_text():
    """The hit world of the remote-command tests -- plain remote bindings -- generates the PARENT commit's text byte for byte (tests/golden/hit_world_*.hip); the
    headline world's text is the committed golden text; the brand world registered with send_insert only names nothing new."""
    for form, steady in (("generic", False), ("steady", True)):
        w = layout_world(); build_hit(w)
        assert w.generated_kernel_source(steady=steady) == open(os.path.join(ROOT, "tests", "golden", f"hit_world_{form}.hip")).read(), form
        w = bg.World(1_000_000, max_depth=9, flags=bg.GGRS_WORLD_LAYOUT_ONLY); cm.build_particles(w)
        assert w.generated_kernel_source(steady=steady) == open(os.path.join(ROOT, "docs", "generated", f"headline_{form}.hip")).read(), form
    w, ids = brand_world(values=False)
    src = w.generated_kernel_source()
    for ident in NEW_IDENTIFIERS: assert ident not in src, ident
    assert "rx_inbox" in src
    assert getattr(w._lib, "ggrs_hip_add_custom_system_values")            # (on the parent the symbol is missing: this test fails there too)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")
@pytest.mark.parametrize("which", ["brand", "brand+spawn", "brand+effects"])
def test_brand_world_compiles_for_gfx950_to_a_native_64_bit_atomic_max_without_scratch(which):
    w, _ = brand_world(with_spawn=which == "brand+spawn", effects=which == "brand+effects")
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
        atomics = [ln.split("//")[0].split() for ln in asm.splitlines() if "global_atomic_" in ln]
        print(which, "steady" if steady else "generic", res, sorted(set(a[0] for a in atomics)))
        maxes = [a for a in atomics if a[0] == "global_atomic_umax_x2"]
        # four value bindings: each key one native 64-bit unsigned max, no compare-and-swap loop, no returned value (no sc0); the ORs as before
        assert 1 <= len(maxes) <= 4, atomics
        assert "global_atomic_cmpswap" not in asm and not any("sc0" in a for a in atomics), atomics
        assert all(a[0] in ("global_atomic_umax_x2", "global_atomic_or", "global_atomic_add", "global_atomic_xor_x2") for a in atomics), atomics
        assert res.get("private_segment_fixed_size") == 0 and res.get("vgpr_spill_count") == 0, res
        assert "scratch_" not in asm and "buffer_wbl2" not in asm and "buffer_inv" not in asm       # no scratch access; the kernel boundary is the only synchronisation


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf")), reason="no hipcc / llvm-readelf")
def test_the_apply_kernels_gather_the_winners_words_without_scratch():
    """rx_apply_unit indexes the payload pointers of its argument block with the winner's ordinal, which differs per lane: that must stay a load from the
    kernel-argument segment, not a copy of the block into scratch.  The library's device code, compiled for gfx950 with the Makefile's flags."""
    csrc = os.path.join(ROOT, "bevy_ggrs_amd", "csrc")
    flags = re.search(r"^HIPFLAGS \?= (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).replace("$(ARCH)", "gfx950").split()
    with tempfile.NamedTemporaryFile(suffix=".hsaco") as f:
        subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--offload-device-only", "--no-gpu-bundle-output", "-c", os.path.join(csrc, "ggrs_hip.hip"), "-o", f.name], check=True, capture_output=True)
        notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
    seen = 0
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_apply_remote" not in name: continue
        res = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\d+)", blk)}
        print(name, res)
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0 and res["vgpr_count"] <= 64, (name, res)
        seen += 1
    assert seen == 2                                                       # k_apply_remote and k_apply_remote_effects


# ---- the oracle sessions of test_gpu_remote_values.py, computed once and shared; the coverage floors --------------------------------------------------------
# name: (slots, check distance (-1: the P2P-shaped lists), ticks, world variant, links)
SCENARIOS = {"1": (1, 7, 12, {}, None), "64": (64, 7, 24, {}, None), "65": (65, 7, 24, {}, None), "257": (257, 7, 24, {}, None), "1025": (1025, 7, 12, {}, None),
             "8262": (8262, 7, 9, {}, None), "8262 all to 0": (8262, 7, 9, {}, all_to_zero_links),
             "floor synctest": (300, 7, 24, {"with_spawn": True}, None), "floor p2p": (300, -1, 0, {"with_spawn": True}, None),
             "effects": (300, 7, 24, {"effects": True}, None)}
DEPTH = 8


def scenario_lists(name):
    n, cd, ticks, kw, links = SCENARIOS[name]
    patch = spawn_patch(n) if kw.get("with_spawn") else None
    if cd < 0: return p2p_lists(patch)
    return synctest_lists(cd, ticks, depth=DEPTH, patch=patch, inputs=lambda t: (t % 3,))


@functools.lru_cache(maxsize=None)
def oracle_session(name):
    """The oracle's session of a scenario: (checksums [(frame, u128)], final state, the oracle world, its ids, its Stats)."""
    n, cd, ticks, kw, links = SCENARIOS[name]
    o = OracleWorld(n + 128, DEPTH, FLAT); st = Stats()
    ids = build_brand(o, n, st=st, **kw); spawn_brand(o, ids, n, links=None if links is None else links(n)); o.set_depth(DEPTH)
    cks = run_oracle(o, scenario_lists(name), cd)
    return cks, cm.snapshot_state(o, ids), o, ids, st


# The floors, as measured on the CPU (the world's moduli were tuned until no counter stayed below 3): a GPU comparison against these sessions cannot pass by never
# exercising a conflict.  The spawn variant: only a world that spawns can hit an entity in the frame it appears.
FLOORS = {"floor synctest": {"val_absent": 4216, "val_present": 13669, "multi_same_binding": 597, "multi_two_bindings_one_system": 1701, "multi_two_systems": 4356, "value_and_default": 2536,
                            "value_and_remove": 1425, "value_and_despawn": 157, "out_of_range": 387, "dead_target": 5778, "spawned_this_frame": 30, "dead_sender": 54,
                            "winner_differs_from_every_loser": 4180},
          "floor p2p": {"val_absent": 1941, "val_present": 4892, "multi_same_binding": 162, "multi_two_bindings_one_system": 680, "multi_two_systems": 1661, "value_and_default": 1002,
                        "value_and_remove": 549, "value_and_despawn": 62, "out_of_range": 377, "dead_target": 1442, "spawned_this_frame": 25, "dead_sender": 13,
                        "winner_differs_from_every_loser": 1565}}


@pytest.mark.parametrize("name", list(FLOORS))
def test_oracle_sessions_reach_every_counter_at_least_three_times(name):
    cks, final, o, ids, st = oracle_session(name)
    fl = st.floors()
    print(name, "frames", st.frames, "sent", st.sent, "landed", st.landed, fl)
    for k, v in fl.items(): assert v >= 3, (name, k, fl)
    assert fl == FLOORS[name], (name, fl)                                                       # the floors as measured
    assert st.landed > 0 and st.sent > 0
    assert "ggrs_hip_add_custom_system_values" in _ffi.SIGNATURES             # (the sessions are the GPU tests' references: without the entry point this test fails too)
    B, M = ids[3], ids[4]
    assert 0 < int(final[f"present{B}"].sum()) < final["len"] and 0 < int(final[f"present{M}"].sum()) and not final["alive"].all()
