"""Deterministic float sums into a device resource (ggrs_hip_add_custom_system_sums: e.sum_f32 / e.sum_f64, the balanced binary tree over slot indices), checked WITHOUT
a GPU on GGRS_WORLD_LAYOUT_ONLY worlds: the entry point exists in every layer that mirrors the ABI; with no sum binding it gives the remote entry point's text byte for
byte; a world without sum bindings names none of the new identifiers; every refusal of include/ggrs_hip.h answers GGRS_E_INVALID with a message naming the system and
the resource; the flock world's generated text keeps one accumulator per summed word at the -0.0 bit pattern, sums it with a DPP ladder of float adds and stores with
one plain store, compiles for gfx950, needs no scratch and adds no atomic; and the Python model beside the oracle has the properties the GPU tests lean on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
import sums_common as sc
from bevy_ggrs_amd import _ffi
from reduces_common import LOOK_SRC, build_census
from test_resources_text import _build, _invalid, _one, _refused, layout_world      # (names only: helpers, no test is imported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMER = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.sum_f32(0, e.f32(0)); }"
NEW_IDENTIFIERS = ("sum_part", "wave_sum32", "wave_sum64", "sm_step32", "sm_step64", "sum_f32", "sum_f64", "ent.smf_[", "ent.smw_[", "ent.sma_[", "GGRS_SM_LADDER", "SUM BINDINGS")
GPU_SIZES = (1, 63, 64, 65, 256, 257, 1025)                          # test_gpu_sums.py's SyncTest shapes
RESET0 = "__device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame&) { r.f32(0) = 0.f; }"


def test_entry_point_exists_in_header_library_ctypes_mirror_rust_shim_and_cpp_mirror():
    hdr = open(os.path.join(ROOT, "include", "ggrs_hip.h")).read()
    rs = open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "bevy_ggrs_hip.hpp")).read()
    lib = C.CDLL(_ffi.LIB_PATH)
    fn = "ggrs_hip_add_custom_system_sums"
    assert re.search(r"\bint %s\(ggrs_world\* w," % fn, hdr)
    assert hasattr(lib, fn) and fn in _ffi.SIGNATURES and ("pub fn %s(w: *mut ggrs_world," % fn) in rs and (fn + "(w, ") in hpp
    # the remote entry point's argument list plus the sum bindings at the end
    assert re.search(r"const ggrs_remote_binding\* rem, uint32_t n_rem,\s*const ggrs_sum_binding\* sum, uint32_t n_sum\);", hdr)
    assert _ffi.SIGNATURES[fn][1][:-2] == _ffi.SIGNATURES["ggrs_hip_add_custom_system_remote"][1]
    assert "sum: *const ggrs_sum_binding, n_sum: u32) -> c_int;" in rs
    assert "typedef struct { uint32_t res; uint32_t word; } ggrs_sum_binding;" in hdr and "pub struct ggrs_sum_binding {" in rs
    assert re.search(r"#define GGRS_SUM_MAX_BINDINGS\s+4\b", hdr) and "pub const GGRS_SUM_MAX_BINDINGS: usize = 4;" in rs and bg.SUM_MAX_BINDINGS == 4
    assert re.search(r"#define GGRS_SUM_MAX_WORDS\s+8\b", hdr) and "pub const GGRS_SUM_MAX_WORDS: usize = 8;" in rs and bg.SUM_MAX_WORDS == 8
    assert C.sizeof(_ffi.SumBinding) == 8
    assert "#define GGRS_HIP_ABI_VERSION 9" in hdr and _ffi.lib.ggrs_hip_abi_version() == 9
    assert "sum_partials" in hdr and hasattr(lib, "ggrs_dbg_sum_partials")
    assert not re.search(r"#define GGRS_REDUCE_(?!MAX_BINDINGS)", hdr)
    # the contract, in full, and the pointer from the reduce paragraph
    for words in ("BALANCED BINARY TREE OVER SLOT INDICES", "a_s starts at -0.0", "level k+1 is x[2i] + x[2i+1]", "the word becomes w + T, ONE add", "With n_sum == 0 the call behaves exactly as",
                  "A NaN operand gives a NaN result whose payload is unspecified", "Subnormals are kept", "float words are not offered", "float SUMS have their",
                  "both a sum binding and a reduce binding", "ggrs_hip_fanout_step works"):
        assert words in hdr, words
    for doc in ("DESIGN.md", "INTEGRATION.md", "README.md"):
        assert fn in open(os.path.join(ROOT, doc)).read(), doc


def _desc(H, src=LOOK_SRC):
    d = _ffi.CustomSystemDesc(); d.name, d.source, d.n_bindings = b"custom", src.encode(), 1; d.comp[0], d.word[0] = H, 0
    return d


def test_zero_sum_bindings_is_the_remote_entry_point():
    texts = []
    for how in ("remote", "sums"):
        w = layout_world(); H = _one(w); R = w.register_resource("Clock", 4, 2)
        d = _desc(H)
        rb = (_ffi.ResourceBinding * 1)(); rb[0].res, rb[0].word = R, 1
        if how == "remote": w._check(w._lib.ggrs_hip_add_custom_system_remote(w._p, C.byref(d), None, 0, None, 0, None, 0, rb, 1, None, 0, None, 0))
        else: w._check(w._lib.ggrs_hip_add_custom_system_sums(w._p, C.byref(d), None, 0, None, 0, None, 0, rb, 1, None, 0, None, 0, None, 0))
        texts.append(w.generated_kernel_source())
    assert texts[0] == texts[1] and "ent.rs_[0] = (ggrs_u64)r1;" in texts[1]
    for ident in NEW_IDENTIFIERS: assert ident not in texts[1], ident
    # ... and through the Python layer: sums=[] goes through the new entry point and changes nothing
    w = layout_world(); H = _one(w); R = w.register_resource("Clock", 4, 2)
    w.add_custom_system(LOOK_SRC, [(H, 0)], resources=[(R, 1)], sums=[])
    assert w.generated_kernel_source() == texts[0]


def test_worlds_without_sum_bindings_keep_their_text():
    for form, steady in (("generic", False), ("steady", True)):
        w = bg.World(1_000_000, max_depth=9, flags=bg.GGRS_WORLD_LAYOUT_ONLY); cm.build_particles(w)
        src = w.generated_kernel_source(steady=steady)
        assert src == open(os.path.join(ROOT, "docs", "generated", f"headline_{form}.hip")).read(), form
        for ident in NEW_IDENTIFIERS: assert ident not in src, ident
    from commands_common import build_stun
    from peer_effects_common import build_strike
    from resources_common import build_clock
    for build in (build_stun, build_strike, build_clock, build_census, lambda w: sc.build_flock(w, variant="plain"), lambda w: sc.build_flock(w, variant="ureduce")):
        w = layout_world(); build(w)
        for steady in (False, True):
            src = w.generated_kernel_source(steady=steady)
            for ident in NEW_IDENTIFIERS: assert ident not in src, ident
    for steady in (False, True):
        w = layout_world(); sc.build_flock(w)
        src = w.generated_kernel_source(steady=steady)
        for ident in NEW_IDENTIFIERS: assert ident in src, ident


def _centre_like(w):
    H = _one(w); Ce = w.register_resource("Centre", 4, 2); En = w.register_resource("Energy", 8, 1)
    return H, Ce, En


def test_refusals_name_the_system_and_the_resource():
    # a reader registered AFTER the summer; the summer reading its own word; a reader and a resetting resource system registered before it are allowed
    w = layout_world(); H, Ce, En = _centre_like(w)
    w.add_custom_system(SUMMER, [(H, 0)], name="tally", sums=[(Ce, 0)])
    w.add_custom_system(LOOK_SRC, [(H, 0)], name="late_look", resources=[(Ce, 0)])
    _refused(w, "'tally'", "'late_look'", "'Centre'", "word 0 of resource 0", "reads through resource binding 0", "at or after the first summer")
    w = layout_world(); H, Ce, En = _centre_like(w)
    w.add_custom_system(SUMMER, [(H, 0)], name="greedy", resources=[(Ce, 0)], sums=[(Ce, 0)])
    _refused(w, "'greedy'", "'Centre'", "at or after the first summer")
    w = layout_world(); H, Ce, En = _centre_like(w)
    w.add_custom_system(LOOK_SRC, [(H, 0)], name="look", resources=[(Ce, 0)])
    w.add_resource_system(RESET0, [(Ce, 0)], name="reset")
    w.add_custom_system(SUMMER, [(H, 0)], name="tally", sums=[(Ce, 0)])
    w.add_custom_system(LOOK_SRC, [(H, 0)], name="other_word", resources=[(Ce, 1)])      # another word of the same resource: no rule
    assert "wave_sum32(sm0)" in w.generated_kernel_source()
    # a resource system registered after the summer
    w = layout_world(); H, Ce, En = _centre_like(w)
    w.add_custom_system(SUMMER, [(H, 0)], name="tally", sums=[(Ce, 1)])
    w.add_resource_system(RESET0, [(Ce, 1)], name="late_reset")
    _refused(w, "'tally'", "resource system 'late_reset'", "'Centre'", "word 1 of resource 0", "at or after the first summer")
    # a word under a sum binding AND a reduce binding, in two systems and in one
    w = layout_world(); H, Ce, En = _centre_like(w)
    w.add_custom_system(SUMMER, [(H, 0)], name="tally", sums=[(Ce, 0)])
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.reduce_u32(0, 1u); }", [(H, 0)], name="count", reduces=[(Ce, 0, bg.EFFECT_ADD)])
    _refused(w, "'tally'", "'count'", "'Centre'", "word 0 of resource 0", "a sum binding or a reduce binding, not both")
    w = layout_world(); H, Ce, En = _centre_like(w)
    w.add_custom_system(SUMMER, [(H, 0)], name="both", reduces=[(En, 0, bg.EFFECT_ADD)], sums=[(En, 0)])
    _refused(w, "'both'", "'Energy'", "a sum binding or a reduce binding, not both")
    # the resource, or the word, does not exist
    w = layout_world(); H, Ce, En = _centre_like(w)
    w.add_custom_system(SUMMER, [(H, 0)], name="tally", sums=[(7, 0)])
    _refused(w, "'tally'", "sum binding 0", "resource 7", "not registered")
    w = layout_world(); H, Ce, En = _centre_like(w)
    w.add_custom_system(SUMMER, [(H, 0)], name="tally", sums=[(En, 1)])
    _refused(w, "'tally'", "word 1 of resource 1", "'Energy'", "has 1 words")
    # more than GGRS_SUM_MAX_BINDINGS per system, more than GGRS_SUM_MAX_WORDS per world
    w = layout_world(); H, Ce, En = _centre_like(w)
    d = _desc(H, SUMMER); d.name = b"many"
    sb = (_ffi.SumBinding * 5)()
    _invalid(lambda: w._check(w._lib.ggrs_hip_add_custom_system_sums(w._p, C.byref(d), None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, sb, 5)), "'many'", "GGRS_SUM_MAX_BINDINGS")
    w = layout_world(); H = _one(w); Wide = w.register_resource("Wide", 4, 9)
    for k in range(3): w.add_custom_system(SUMMER, [(H, 0)], name=f"part{k}", sums=[(Wide, 3 * k + j) for j in range(3)])
    _refused(w, "'part2'", "'Wide'", "GGRS_SUM_MAX_WORDS")
    # everything device resources refuse: a world that keeps RollbackDespawned markers, one without the generated kernel
    w = layout_world(); H, Ce, En = _centre_like(w)
    w.add_custom_system(SUMMER, [(H, 0)], name="tally", sums=[(Ce, 0)])
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, bg.DESPAWN_ROLLBACK))
    _refused(w, "device resources", "'Centre'", "RollbackDespawned markers")
    w = layout_world(flags=bg.GGRS_WORLD_NO_GROUPS); H, Ce, En = _centre_like(w)
    w.add_custom_system(SUMMER, [(H, 0)], name="tally", sums=[(Ce, 0)])
    _refused(w, "device resources", "'Centre'", "need the generated request-group kernel")
    # op 8 through a REDUCE binding is still refused, with the message it has
    w = layout_world(); H, Ce, En = _centre_like(w)
    _invalid(lambda: w.add_custom_system(SUMMER, [(H, 0)], name="count", reduces=[(Ce, 0, 8)]), "'count'", "reduce binding 0", "op 8", "GGRS_EFFECT_")


def test_flock_text_accumulates_in_registers_and_stores_once_per_wave():
    w = layout_world(); sc.build_flock(w)
    src = w.generated_kernel_source()
    body = src.split('extern "C" __global__')[1]
    head = body[:body.index("for (uint32_t op = 0;")]
    # one per-lane accumulator per summed word at -0.0 AS A BIT PATTERN, ahead of the op loop: registers Centre.sx r0, Centre.sy r1, Energy.e r2
    for line in ("float sm0 = __uint_as_float(0x80000000u);", "float sm1 = __uint_as_float(0x80000000u);", "double sm2 = __longlong_as_double((long long)0x8000000000000000ull);"):
        assert head.count(line) == 1 and body.count(line) == 1, line
    assert "-0.0f" not in body and "= 0.0" not in head
    # handed to the system typed, taken back after the call -- tally (system 2) and the second summer of sx (system 3)
    assert ("ent.smf_[0] = sm0; ent.smw_[0] = 4u; ent.sma_[0] = 0u;\n                ent.smf_[1] = sm1; ent.smw_[1] = 4u; ent.sma_[1] = 1u;\n"
            "                ent.smd_[2] = sm2; ent.smw_[2] = 8u; ent.sma_[2] = 2u;\n") in body
    assert "                sm0 = ent.smf_[0];\n                sm1 = ent.smf_[1];\n                sm2 = ent.smd_[2];\n" in body
    assert body.count("ent.smf_[0] = sm0; ent.smw_[0] = 4u; ent.sma_[0] = 0u;") == 2 and body.count("sm0 = ent.smf_[0];") == 2
    # e.sum_* touches no memory: behind the op loop and the live store, one ladder and ONE plain store per word, by lane 63, unconditional; the only atomic is Census.alive's
    tail = body[body.index("// ---- the live world, written once"):]
    assert body.count("__hip_atomic_fetch_") == tail.count("__hip_atomic_fetch_") == 1 and "__hip_atomic_fetch_add((GGRS_G uint32_t*)" in tail
    for line in ("{ const float v_ = wave_sum32(sm0);\n          if (lane == 63u) *(GGRS_G float*)(a.sum_part + (0ull + (uint64_t)gu * 8ull)) = v_; }",
                 "{ const float v_ = wave_sum32(sm1);\n          if (lane == 63u) *(GGRS_G float*)(a.sum_part + (1024ull + (uint64_t)gu * 8ull)) = v_; }",
                 "{ const double v_ = wave_sum64(sm2);\n          if (lane == 63u) *(GGRS_G double*)(a.sum_part + (2048ull + (uint64_t)gu * 8ull)) = v_; }"):
        assert tail.count(line) == 1 and body.count(line) == 1, line
    assert "atomicCAS" not in body and "compare_exchange" not in src and "s_sleep" not in body
    # the ladder is wave_xor32's lane pattern with -0.0 as `old` and a float add
    for ctrl in ("0xB1, 0xF", "0x4E, 0xF", "0x141, 0xF", "0x140, 0xF", "0x142, 0xA", "0x143, 0xC"): assert f"STEP<{ctrl}>(v);" in src, ctrl
    assert "return v + __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp((int)0x80000000u, (int)__float_as_uint(v), CTRL, ROWS, 0xF, false));" in src
    assert "__builtin_amdgcn_update_dpp((int)0x80000000u, (int)(uint32_t)(b_ >> 32), CTRL, ROWS, 0xF, false)" in src
    # one AdvanceWorld per launch; the pointer is an argument, and stays one in a specialised copy
    assert "unsigned char* sum_part;" in src
    steady = w.generated_kernel_source(steady=True)
    assert steady.startswith("#define GGRS_SPEC 1\n") and "a.sum_part + (1024ull + (uint64_t)gu * 8ull)" in steady and "unsigned char* sum_part;" in steady


def test_second_binding_of_one_word_in_one_system_shares_the_accumulator():
    w = layout_world(); H, Ce, En = _centre_like(w)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.sum_f32(0, 1.f); e.sum_f32(1, 2.f); e.sum_f64(0, 1.0); e.sum_f32(3, 1.f); }", [(H, 0)], name="twice",
                        sums=[(Ce, 0), (Ce, 0)])
    body = w.generated_kernel_source().split('extern "C" __global__')[1]
    assert "ent.smf_[0] = sm0; ent.smw_[0] = 4u; ent.sma_[0] = 0u;\n                ent.smw_[1] = 4u; ent.sma_[1] = 0u;\n" in body and body.count("sm0 = ent.smf_") == 1


def test_a_summer_cannot_read_the_running_value():
    w = layout_world(); H, Ce, En = _centre_like(w)
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.f32(0) = e.sum_f32(0, 1.f); }", [(H, 0)], name="peek", sums=[(Ce, 0)])
    assert e.value.code == bg.GGRS_E_INVALID and "custom system 'peek' does not compile" in str(e.value), str(e.value)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")
@pytest.mark.parametrize("steady", [False, True])
def test_flock_world_compiles_for_gfx950_without_scratch_or_new_atomics(steady):
    """The .vgpr_count / .sgpr_count of the flock world and of the same world without sum bindings are printed here and recorded in profiles/float_sums/README.md and
    DESIGN 3.11; no bound on them is fixed -- only: no scratch, no spills, exactly the atomics the u32 reducer has without the sum bindings, float adds behind DPP moves."""
    out = {}
    for which in ("sums", "plain"):
        w = layout_world(); sc.build_flock(w, variant=which)
        res, asm = _build(w.generated_kernel_source(steady=steady, compile=True))
        print(which, "steady" if steady else "generic", res)
        assert res.get("private_segment_fixed_size") == 0 and res.get("vgpr_spill_count") == 0, (which, res)
        assert "scratch_" not in asm and "cmpswap" not in asm, which
        out[which] = (res, asm)
    assert out["sums"][1].count("global_atomic") == out["plain"][1].count("global_atomic") == 1
    asm = out["sums"][1]
    assert "v_add_f32" in asm and "v_add_f64" in asm and "row_bcast:15" in asm and "row_bcast:31" in asm and "row_mirror" in asm
    assert "v_add_f64" not in out["plain"][1]
    readme = open(os.path.join(ROOT, "profiles", "float_sums", "README.md")).read()
    form = "steady" if steady else "generic"
    for which in ("sums", "plain"):
        assert re.search(r"\| %s \| %s \| %d \| %d \|" % (which, form, out[which][0]["vgpr_count"], out[which][0]["sgpr_count"]), readme), (which, form, out[which][0])


# ---- the model's own properties ---------------------------------------------------------------------------------------------------------------------------------
def test_tree_sum_does_not_depend_on_padding():
    for n in (1, 2, 3, 63, 64, 65, 257, 1025):
        for dt in (sc.F32, sc.F64):
            a = sc.order_values(n).astype(dt)
            want = sc.bits_of(sc.tree_sum(a))
            for pad in (1, 63, 64, 191, 3000):
                assert sc.bits_of(sc.tree_sum(np.concatenate([a, np.full(pad, -0.0, dtype=dt)]))) == want, (n, dt, pad)
    assert sc.f32_bits(sc.tree_sum(np.zeros(0, dtype=sc.F32))) == sc.NEG_ZERO_32


def test_a_frame_without_calls_returns_the_words_bits():
    layout = [("A", 4, [(sc.f32_bits(0.0), sc.SUM), (sc.NEG_ZERO_32, sc.SUM), (sc.f32_bits(1e-42), sc.SUM)]), ("B", 8, [(sc.f64_bits(0.0), sc.SUM), (sc.NEG_ZERO_64, sc.SUM), (sc.f64_bits(-3.25), sc.SUM)])]
    m = sc.SumModel(layout, 130)
    before = m.words()
    m.begin(0); m.end()
    assert m.words() == before and before[0][0] == 0 and before[0][1] == 0x80000000 and 0 < before[0][2] < 0x00800000      # +0.0, -0.0 and a subnormal keep their bits
    m.begin(0); m.sum(0, 0, 5, 1.5); m.sum(0, 0, 5, 2.25); m.sum(1, 2, 129, 0.25); m.end()
    assert m.cur[0][0] == sc.f32_bits(3.75) and m.cur[1][2] == sc.f64_bits(-3.0) and m.cur[0][1] == 0x80000000


@pytest.mark.parametrize("n", [n for n in GPU_SIZES if n >= 63] + [255, 513, 4099])
def test_order_matters_for_the_inputs_the_gpu_tests_use(n):
    """Otherwise the GPU tests would prove nothing: for the x and y the flock starts with, at every SyncTest size, the tree's bits differ from the slot-order sum, the
    reverse-order sum and sequential-per-64-then-sequential."""
    x, y = sc.flock_xy(0, n)
    assert (x == sc.order_values(n)).all()
    for name, a in (("x", x), ("y", y)):
        t = sc.f32_bits(sc.tree_sum(a))
        others = [sc.f32_bits(v) for v in sc.other_orders(a)]
        assert t not in others, (n, name, hex(t), [hex(o) for o in others])
