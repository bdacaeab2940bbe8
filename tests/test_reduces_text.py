"""Entity systems that reduce into a device resource (ggrs_hip_add_custom_system_reduces: e.reduce_u32 / _i32 / _u64), checked WITHOUT a GPU on
GGRS_WORLD_LAYOUT_ONLY worlds: the entry point exists in every layer that mirrors the ABI; with no reduce binding it gives the resources entry point's text byte for
byte; a world without reducers names none of the new identifiers; every refusal of include/ggrs_hip.h answers GGRS_E_INVALID with a message naming the system and the
resource; the census world's generated text keeps one accumulator per reduced word, reduces it with a DPP ladder and publishes with one no-return atomic, compiles for
gfx950, needs no scratch and holds no compare-and-swap."""
import ctypes as C
import os
import re

import pytest

import bevy_ggrs_amd as bg
import common as cm
from bevy_ggrs_amd import _ffi
from reduces_common import COUNT_SRC, LOOK_SRC, build_census, build_ops
from test_resources_text import _build, _invalid, _one, _refused, layout_world      # (names only: helpers, no test is imported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOP = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) += 1u; }"
RED = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.reduce_u32(0, e.u32(0)); }"
NEW_IDENTIFIERS = ("rd_inbox", "wave_reduce32", "wave_reduce64", "rd_step32", "rd_comb", "reduce_u32", "reduce_u64", "ent.rd_[", "ent.rdw_[", "ent.rdo_[", "GGRS_RD_LADDER", "REDUCE BINDINGS")


def test_entry_point_exists_in_header_library_ctypes_mirror_and_rust_shim():
    hdr = open(os.path.join(ROOT, "include", "ggrs_hip.h")).read()
    rs = open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "bevy_ggrs_hip.hpp")).read()
    lib = C.CDLL(_ffi.LIB_PATH)
    fn = "ggrs_hip_add_custom_system_reduces"
    assert re.search(r"\bint %s\(ggrs_world\* w," % fn, hdr)
    assert hasattr(lib, fn) and fn in _ffi.SIGNATURES and ("pub fn %s(w: *mut ggrs_world," % fn) in rs and (fn + "(w, ") in hpp
    # the resources entry point's argument list plus the reduce bindings at the end
    assert re.search(r"const ggrs_resource_binding\* res, uint32_t n_res,\s*const ggrs_reduce_binding\* red, uint32_t n_red\);", hdr)
    assert _ffi.SIGNATURES[fn][1][:-2] == _ffi.SIGNATURES["ggrs_hip_add_custom_system_resources"][1]
    assert "red: *const ggrs_reduce_binding, n_red: u32) -> c_int;" in rs
    assert "typedef struct { uint32_t res; uint32_t word; uint32_t op; } ggrs_reduce_binding;" in hdr and "pub struct ggrs_reduce_binding {" in rs
    assert re.search(r"#define GGRS_REDUCE_MAX_BINDINGS\s+8\b", hdr) and "pub const GGRS_REDUCE_MAX_BINDINGS: usize = 8;" in rs and bg.REDUCE_MAX_BINDINGS == 8
    assert C.sizeof(_ffi.ReduceBinding) == 12
    assert "#define GGRS_HIP_ABI_VERSION 9" in hdr and _ffi.lib.ggrs_hip_abi_version() == 9
    assert "reduce_inbox" in hdr
    # the op codes are reused: no new op constants
    assert not re.search(r"#define GGRS_REDUCE_(?!MAX_BINDINGS)", hdr)
    for words in ("WRITING or reducing into a resource", "The sentence above narrows here", "ALL REDUCTIONS OF A FRAME LAND AT THE END OF THE FRAME",
                  "a reducer cannot read the running value", "An accessor of the wrong width for its word does nothing", "also in the call that despawns its entity",
                  "a word has one op in the whole world", "With n_red == 0 the call behaves exactly as", "float words are not offered", "ggrs_hip_fanout_step works"):
        assert words in hdr, words


def test_zero_reduce_bindings_is_the_resources_entry_point():
    texts = []
    for how in ("resources", "reduces"):
        w = layout_world(); H = _one(w); R = w.register_resource("Clock", 4, 2)
        d = _ffi.CustomSystemDesc(); d.name, d.source, d.n_bindings = b"custom", LOOK_SRC.encode(), 1; d.comp[0], d.word[0] = H, 0
        rb = (_ffi.ResourceBinding * 1)(); rb[0].res, rb[0].word = R, 1
        if how == "resources": w._check(w._lib.ggrs_hip_add_custom_system_resources(w._p, C.byref(d), None, 0, None, 0, None, 0, rb, 1))
        else: w._check(w._lib.ggrs_hip_add_custom_system_reduces(w._p, C.byref(d), None, 0, None, 0, None, 0, rb, 1, None, 0))
        texts.append(w.generated_kernel_source())
    assert texts[0] == texts[1] and "ent.rs_[0] = (ggrs_u64)r1;" in texts[1]
    for ident in NEW_IDENTIFIERS: assert ident not in texts[1], ident


def test_worlds_without_reducers_keep_their_text():
    for form, steady in (("generic", False), ("steady", True)):
        w = bg.World(1_000_000, max_depth=9, flags=bg.GGRS_WORLD_LAYOUT_ONLY); cm.build_particles(w)
        src = w.generated_kernel_source(steady=steady)
        assert src == open(os.path.join(ROOT, "docs", "generated", f"headline_{form}.hip")).read(), form
        for ident in NEW_IDENTIFIERS: assert ident not in src, ident
    from commands_common import build_stun
    from peer_effects_common import build_strike
    from resources_common import build_clock
    for build in (build_stun, build_strike, build_clock, lambda w: build_census(w, plain=True)):
        w = layout_world(); build(w)
        src = w.generated_kernel_source()
        for ident in NEW_IDENTIFIERS: assert ident not in src, ident
    w = layout_world(); build_census(w)
    src = w.generated_kernel_source()
    for ident in NEW_IDENTIFIERS: assert ident in src, ident


def _census_like(w):
    H = _one(w); Cn = w.register_resource("Census", 4, 2); To = w.register_resource("Total", 8, 1)
    return H, Cn, To


def test_refusals_name_the_system_and_the_resource():
    # a reader registered AFTER the reducer; the reducer reading its own word; a reader registered before it is allowed
    w = layout_world(); H, Cn, To = _census_like(w)
    w.add_custom_system(RED, [(H, 0)], name="count", reduces=[(Cn, 0, bg.EFFECT_ADD)])
    w.add_custom_system(LOOK_SRC, [(H, 0)], name="late_look", resources=[(Cn, 0)])
    _refused(w, "'count'", "'late_look'", "'Census'", "word 0 of resource 0", "reads through resource binding 0", "at or after the first reducer")
    w = layout_world(); H, Cn, To = _census_like(w)
    w.add_custom_system(RED, [(H, 0)], name="greedy", resources=[(Cn, 0)], reduces=[(Cn, 0, bg.EFFECT_ADD)])
    _refused(w, "'greedy'", "'Census'", "at or after the first reducer")
    w = layout_world(); H, Cn, To = _census_like(w)
    w.add_custom_system(LOOK_SRC, [(H, 0)], name="look", resources=[(Cn, 0)])
    w.add_resource_system("__device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame&) { r.u32(0) = 0u; }", [(Cn, 0)], name="reset")
    w.add_custom_system(RED, [(H, 0)], name="count", reduces=[(Cn, 0, bg.EFFECT_ADD)])
    w.add_custom_system(LOOK_SRC, [(H, 0)], name="other_word", resources=[(Cn, 1)])      # another word of the same resource: no rule
    assert "wave_reduce32<0u>" in w.generated_kernel_source()
    # a resource system registered after the reducer
    w = layout_world(); H, Cn, To = _census_like(w)
    w.add_custom_system(RED, [(H, 0)], name="count", reduces=[(Cn, 1, bg.EFFECT_OR)])
    w.add_resource_system("__device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame&) { r.u32(0) = 0u; }", [(Cn, 1)], name="late_reset")
    _refused(w, "'count'", "resource system 'late_reset'", "'Census'", "word 1 of resource 0", "at or after the first reducer")
    # two ops on one word, in two systems and in one
    w = layout_world(); H, Cn, To = _census_like(w)
    w.add_custom_system(RED, [(H, 0)], name="adder", reduces=[(Cn, 0, bg.EFFECT_ADD)])
    w.add_custom_system(RED, [(H, 0)], name="maxer", reduces=[(Cn, 0, bg.EFFECT_MAX_U)])
    _refused(w, "'maxer'", "'Census'", "GGRS_EFFECT_MAX_U", "GGRS_EFFECT_ADD", "a word has one op in the whole world")
    w = layout_world(); H, Cn, To = _census_like(w)
    w.add_custom_system(RED, [(H, 0)], name="both", reduces=[(To, 0, bg.EFFECT_XOR), (To, 0, bg.EFFECT_AND)])
    _refused(w, "'both'", "'Total'", "GGRS_EFFECT_AND", "GGRS_EFFECT_XOR", "one op")
    # the resource, or the word, does not exist
    w = layout_world(); H, Cn, To = _census_like(w)
    w.add_custom_system(RED, [(H, 0)], name="count", reduces=[(7, 0, bg.EFFECT_ADD)])
    _refused(w, "'count'", "reduce binding 0", "resource 7", "not registered")
    w = layout_world(); H, Cn, To = _census_like(w)
    w.add_custom_system(RED, [(H, 0)], name="count", reduces=[(To, 1, bg.EFFECT_ADD)])
    _refused(w, "'count'", "word 1 of resource 1", "'Total'", "has 1 words")
    # an op that is none of the eight; more than GGRS_REDUCE_MAX_BINDINGS
    w = layout_world(); H, Cn, To = _census_like(w)
    _invalid(lambda: w.add_custom_system(RED, [(H, 0)], name="count", reduces=[(Cn, 0, 8)]), "'count'", "reduce binding 0", "resource 0", "op 8", "GGRS_EFFECT_")
    d = _ffi.CustomSystemDesc(); d.name, d.source, d.n_bindings = b"many", RED.encode(), 1; d.comp[0], d.word[0] = H, 0
    db = (_ffi.ReduceBinding * 9)()
    _invalid(lambda: w._check(w._lib.ggrs_hip_add_custom_system_reduces(w._p, C.byref(d), None, 0, None, 0, None, 0, None, 0, db, 9)), "'many'", "GGRS_REDUCE_MAX_BINDINGS")
    # everything device resources refuse: a world that keeps RollbackDespawned markers, one without the generated kernel
    w = layout_world(); H, Cn, To = _census_like(w)
    w.add_custom_system(RED, [(H, 0)], name="count", reduces=[(Cn, 0, bg.EFFECT_ADD)])
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, bg.DESPAWN_ROLLBACK))
    _refused(w, "device resources", "'Census'", "RollbackDespawned markers")
    w = layout_world(flags=bg.GGRS_WORLD_NO_GROUPS); H, Cn, To = _census_like(w)
    w.add_custom_system(RED, [(H, 0)], name="count", reduces=[(Cn, 0, bg.EFFECT_ADD)])
    _refused(w, "device resources", "'Census'", "need the generated request-group kernel")


def test_census_text_accumulates_in_registers_and_publishes_once_per_wave():
    w = layout_world(); build_census(w)
    src = w.generated_kernel_source()
    body = src.split('extern "C" __global__')[1]
    head = body[:body.index("for (uint32_t op = 0;")]
    # one per-lane accumulator per reduced word, at the op's identity, ahead of the op loop: registers Census.alive r0, Census.flags r1, Low.hp r2, Total.hp_sum r3
    for line in ("uint32_t rd0 = 0x0u;", "uint32_t rd1 = 0x0u;", "uint32_t rd2 = 0xffffffffu;", "uint64_t rd3 = 0x0ull;"):
        assert head.count(line) == 1 and body.count(line) == 1, line
    # handed to the system with the word's bytes and the op as literals, taken back after the call -- inside the liveness / presence test of the system
    assert "ent.rd_[0] = rd1; ent.rdw_[0] = 4u; ent.rdo_[0] = 5u;\n                ggrs_sys_1::ggrs_system(ent, fr2);\n                rd1 = (uint32_t)ent.rd_[0];" in body
    assert ("ent.rd_[0] = rd0; ent.rdw_[0] = 4u; ent.rdo_[0] = 0u;\n                ent.rd_[1] = rd2; ent.rdw_[1] = 4u; ent.rdo_[1] = 1u;\n"
            "                ent.rd_[2] = rd3; ent.rdw_[2] = 8u; ent.rdo_[2] = 0u;\n                ggrs_sys_2::ggrs_system(ent, fr3);\n"
            "                rd0 = (uint32_t)ent.rd_[0];\n                rd2 = (uint32_t)ent.rd_[1];\n                rd3 = (uint64_t)ent.rd_[2];") in body
    # e.reduce_* touches no memory: the only atomics of the text are the four publications, behind the op loop and the live store, one lane each, skipped at the identity
    tail = body[body.index("// ---- the live world, written once"):]
    assert body.count("__hip_atomic_fetch_") == tail.count("__hip_atomic_fetch_") == 4
    assert "unsigned char* const rl_ = a.rd_inbox + (tile % 64u) * 64u;" in tail
    for line in ("{ const uint32_t v_ = wave_reduce32<0u>(0x0u, rd0);\n          if (lane == 0u && v_ != 0x0u) (void)__hip_atomic_fetch_add((GGRS_G uint32_t*)(rl_ + 8u), (uint32_t)v_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }",
                 "{ const uint32_t v_ = wave_reduce32<5u>(0x0u, rd1);\n          if (lane == 0u && v_ != 0x0u) (void)__hip_atomic_fetch_or((GGRS_G uint32_t*)(rl_ + 12u), (uint32_t)v_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }",
                 "{ const uint32_t v_ = wave_reduce32<1u>(0xffffffffu, rd2);\n          if (lane == 0u && v_ != 0xffffffffu) (void)__hip_atomic_fetch_min((GGRS_G uint32_t*)(rl_ + 16u), (uint32_t)v_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }",
                 "{ const uint64_t v_ = wave_reduce64<0u>(0x0ull, rd3);\n          if (lane == 0u && v_ != 0x0ull) (void)__hip_atomic_fetch_add((GGRS_G uint64_t*)(rl_ + 0u), (uint64_t)v_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }"):
        assert tail.count(line) == 1, line
    assert "atomicCAS" not in body and "compare_exchange" not in src and "s_sleep" not in body
    # the ladder is wave_xor32's lane pattern with the identity as `old`
    for ctrl in ("0xB1, 0xF", "0x4E, 0xF", "0x141, 0xF", "0x140, 0xF", "0x142, 0xA", "0x143, 0xC"): assert f"STEP<OP, {ctrl}>(id, v);" in src, ctrl
    assert "__builtin_amdgcn_update_dpp((int)id, (int)v, CTRL, ROWS, 0xF, false)" in src
    # one AdvanceWorld per launch; the inbox pointer is an argument, and stays one in a specialised copy
    assert "unsigned char* rd_inbox;" in src
    steady = w.generated_kernel_source(steady=True)
    assert steady.startswith("#define GGRS_SPEC 1\n") and "a.rd_inbox + (tile % 64u) * 64u" in steady
    # signed ops publish through the signed atomic; the stripe count is the knob's
    w = layout_world(); build_ops(w, 8)
    src8 = w.generated_kernel_source()
    assert "__hip_atomic_fetch_min((GGRS_G long long*)(rl_ + 24u), (long long)v_," in src8 and "__hip_atomic_fetch_max((GGRS_G long long*)(rl_ + 32u), (long long)v_," in src8
    assert "wave_reduce64<3u>(0x7fffffffffffffffull, rd3)" in src8 and "wave_reduce64<4u>(0x8000000000000000ull, rd4)" in src8


def test_stripe_count_is_one_constant_that_a_debug_call_can_change():
    w = layout_world(); assert w._lib.ggrs_dbg_set_reduce_stripes(w._p, 8) == 0 and w._lib.ggrs_dbg_set_reduce_stripes(w._p, 65) == -1
    build_census(w)
    assert "a.rd_inbox + (tile % 8u) * 64u" in w.generated_kernel_source()


def test_second_binding_of_one_word_in_one_system_is_combined_on_the_way_out():
    w = layout_world(); H, Cn, To = _census_like(w)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.reduce_u32(0, 1u); e.reduce_u32(1, 2u); }", [(H, 0)], name="twice",
                        reduces=[(Cn, 0, bg.EFFECT_ADD), (Cn, 0, bg.EFFECT_ADD)])
    body = w.generated_kernel_source().split('extern "C" __global__')[1]
    assert "ent.rd_[1] = 0x0u; ent.rdw_[1] = 4u; ent.rdo_[1] = 0u;" in body and "rd0 = rd_comb<0u, uint32_t, int>(rd0, (uint32_t)ent.rd_[1]);" in body


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")
@pytest.mark.parametrize("steady", [False, True])
def test_census_world_compiles_for_gfx950_without_scratch_or_cmpswap(steady):
    """The .vgpr_count / .sgpr_count of the census world and of the same world without reducers are printed here and recorded in profiles/resource_reduces/README.md;
    no bound on them is fixed -- only: no scratch, no vector-register spills, no compare-and-swap, native no-return atomics, DPP moves."""
    out = {}
    for which in ("census", "plain"):
        w = layout_world(); build_census(w, plain=which == "plain")
        res, asm = _build(w.generated_kernel_source(steady=steady, compile=True))
        print(which, "steady" if steady else "generic", res)
        assert res.get("private_segment_fixed_size") == 0 and res.get("vgpr_spill_count") == 0, (which, res)
        assert "scratch_" not in asm and "cmpswap" not in asm, which
        if which == "census":
            for insn in ("global_atomic_add ", "global_atomic_or ", "global_atomic_umin ", "global_atomic_add_x2 "): assert insn in asm, insn
            for line in asm.splitlines():
                if "global_atomic" in line: assert " sc0" not in line and " glc" not in line, "an atomic that returns its old value: " + line
            assert "row_bcast:15" in asm and "row_bcast:31" in asm and "row_mirror" in asm
        else: assert "global_atomic" not in asm
        out[which] = res
    readme = open(os.path.join(ROOT, "profiles", "resource_reduces", "README.md")).read()
    form = "steady" if steady else "generic"
    for which in ("census", "plain"):
        assert re.search(r"\| %s \| %s \| %d \| %d \|" % (which, form, out[which]["vgpr_count"], out[which]["sgpr_count"]), readme), (which, form, out[which])


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")
@pytest.mark.parametrize("wb", [4, 8])
def test_all_eight_ops_compile_to_native_atomics(wb):
    w = layout_world(); build_ops(w, wb)
    res, asm = _build(w.generated_kernel_source(compile=True))
    assert res.get("private_segment_fixed_size") == 0 and res.get("vgpr_spill_count") == 0, res
    assert "scratch_" not in asm and "cmpswap" not in asm
    sfx = "_x2 " if wb == 8 else " "
    for op in ("add", "umin", "umax", "smin", "smax", "or", "and", "xor"): assert f"global_atomic_{op}{sfx}" in asm, op


def test_a_reducer_cannot_read_the_running_value():
    """e.reduce_* returns nothing: using its result does not compile."""
    w = layout_world(); H, Cn, To = _census_like(w)
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) = e.reduce_u32(0, 1u); }", [(H, 0)], name="peek", reduces=[(Cn, 0, bg.EFFECT_ADD)])
    assert e.value.code == bg.GGRS_E_INVALID and "custom system 'peek' does not compile" in str(e.value), str(e.value)
    # ... and a system without reduce bindings in a world that has some elsewhere compiles and reduces nothing
    w.add_custom_system(COUNT_SRC, [(H, 0)], name="count", reduces=[(Cn, 0, bg.EFFECT_ADD), (Cn, 1, bg.EFFECT_MIN_U), (To, 0, bg.EFFECT_ADD)])
    w.add_custom_system(NOP, [(H, 0)], name="nop")
    assert "ggrs_sys_1::ggrs_system(ent, fr1);" in w.generated_kernel_source()
