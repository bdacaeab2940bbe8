"""The request-group kernel the library writes per world (ggrs_hip_generated_kernel_source) -- checked WITHOUT a GPU:
a GGRS_WORLD_LAYOUT_ONLY world carries registration + layout only, and hiprtc cross-compiles for gfx950 on any host.
What is pinned here: the generator covers the reference's example schemas (stress_test particles.rs:187-240, box_game
box_game.rs:154-206, tests/synctest.rs:26-52 + despawn_rollback) and user-written systems, its output builds, and the shared device text (device_prelude.hpp) is what both the static and the generated kernels compile.
The numerics of the generated kernel are the `-m gpu` parity suites: it is the default path of every fused world there."""
import os
import re

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dry(capacity=100_000, depth=8):
    return bg.World(capacity, max_depth=depth, flags=bg.GGRS_WORLD_LAYOUT_ONLY)


def particles():
    w = dry()
    cm.build_particles(w, with_spawn=True)
    return w


def box_game(player_rollback):
    w = dry(4)
    T = w.register_component("Transform", 4, 10)
    V = w.register_component("Velocity", 4, 3)
    P = w.register_component("Player", 8, 1, rollback=player_rollback)
    w.checksum_component(T, [0, 1, 2]); w.checksum_component(V, [0, 1, 2])
    w.add_system(bg.SYS_BOX_MOVE, comp=(T, V, P), word=(0, 0, 0), fparam=(18.0, 5.0, 0.0018, 4.5))
    return w


def health(mode):
    w = dry(300)
    H = w.register_component("Health", 4, 1)
    w.register_component("Mesh", 4, 2, rollback=False)
    w.checksum_component(H, [0])
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, mode))
    return w


def custom():
    w = dry()
    H = w.register_component("Health", 4, 1)
    L = w.register_component("Ttl", 8, 1)
    w.checksum_component(H, [0]); w.checksum_component(L, [0])
    w.add_system(bg.SYS_ADD_U32, comp=(H,), word=(0,), iparam=(3,))
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) { e.u32(0) += f.input[0]; if (e.u64(1)-- == 1) e.despawn_rollback(); }",
                        [(H, 0), (L, 0)], name="weird name: \"x\"")
    return w


WORLDS = {"particles": particles, "box_game": lambda: box_game(True), "box_game_live_only_player": lambda: box_game(False),
          "health_despawn": lambda: health(bg.DESPAWN_IMMEDIATE), "health_despawn_rollback": lambda: health(bg.DESPAWN_ROLLBACK), "custom": custom}


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_generated_kernel_builds_for_gfx950(name):
    w = WORLDS[name]()
    src = w.generated_kernel_source(compile=True)      # raises with the hiprtc log if it does not build
    assert 'extern "C" __global__' in src and "ggrs_jit_tick" in src
    assert "sea_diffuse" in src and "box_move_math" in src, "the shared device prelude is part of every generated unit"
    assert "#error" not in src
    if name.endswith("rollback") or name == "custom":
        assert "dis_0" in src and "df_0" in src, "RollbackDespawned markers are carried when a system can defer a despawn"
    else:
        assert "dis_0" not in src
    body = src.split('#line 1 "ggrs_jit_tick"')[1]
    assert "a.parts[at_]" in body and "ff_fold_row(" in body and "__launch_bounds__(256)" in body, "one 256-slot workgroup per tile; the first workgroups fold the previous launch's rows forward"
    assert "static_assert(sizeof(GgrsJitArgs) == " in src and src.count("static_assert(__builtin_offsetof(GgrsJitArgs, ") >= 30, "the per-world argument block is pinned field by field"
    # the argument block carries only what this world's kernel reads
    args = src[src.index("struct GgrsJitArgs {"):src.index("static_assert(sizeof(GgrsJitArgs)")]
    assert ("spawn_payload" in args) == (name == "particles") and ("inputs[" in args) == (name.startswith("box_game") or name == "custom") and ("aux_bits" in args) == name.startswith("box_game")
    assert ("step_flags" in args) == (name.endswith("rollback") or name == "custom")
    if name == "box_game_live_only_player":
        assert "side_h0_0" in src, "a live-only Player.handle is read from the live block, not from the snapshot"


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_kernel_specialised_for_the_steady_tick_builds(name):
    """GGRS_KERNEL_FORM_STEADY: the per-tile form with the SyncTest tick's op sequence, row masks and store policies as literals and
    the op loop unrolled (kernel_gen.hpp jit_specialise) -- the text a running session gets from a worker thread after 16 identical
    groups.  It must build for gfx950 (overwriting fields of the by-value argument struct instead makes the backend abort), keep the
    argument block, and no longer ask the arguments for anything the shape fixes."""
    w = WORLDS[name]()
    gen = w.generated_kernel_source()
    src = w.generated_kernel_source(compile=True, steady=True)
    body = src[src.index('extern "C" __global__'):]
    assert "// specialised: " in src and "#pragma unroll\n    for (uint32_t op = 0; op < " in body
    for field in ("a.op_bits", "a.n_ops", "a.n_saves", "a.save_rows[si]", "a.save_pmask[si]", "a.live_rows", "a.load_rows", "a.nt", "a.dp_s", "a.cached_saves", "a.skip_live"):
        assert field in gen and field not in body, field
    assert "a.save_dst[si]" in body and "a.dt_bits[sj]" in body and "a.len" in body       # what stays an argument
    assert src.startswith("#define GGRS_SPEC 1\n")                 # what lets the text tell an unrolled copy from the general kernel (value tags: destination tags loaded up front)
    assert src[len("#define GGRS_SPEC 1\n"):src.index('extern "C" __global__')].replace(src[src.index("// specialised: "):src.index('extern "C" __global__')], "") == gen[:gen.index('extern "C" __global__')]


# the argument-block fields a specialised kernel turns into literals: kernel_gen.hpp kJitShapeScalars / kJitShapeArrays
SHAPE_SCALARS = ("op_bits", "n_ops", "n_saves", "n_steps", "src_is_live", "skip_live", "dp_s", "nt", "cached_saves", "live_rows", "load_rows", "live_pmask", "nt_loads", "mtab", "vtags")
SHAPE_ARRAYS = ("save_rows", "save_pmask")


def _worlds_incl_schemas():
    out = dict(WORLDS)
    for schema in ("headline", "full", "allhot"):
        def mk(schema=schema):
            w = dry(1_000_000, 9)
            cm.build_particles(w, schema=schema)
            return w
        out["stress_test_" + schema] = mk
    return out


@pytest.mark.parametrize("name", sorted(_worlds_incl_schemas()))
def test_specialiser_substitutes_whole_tokens_and_nothing_else(name):
    """jit_specialise rewrites the generic text; VERDICT r3 (weak 9): a replace keyed on spellings would corrupt a longer identifier
    (`a.nt` inside a future `a.nt_x`) or miss a new use.  For every schema the reference's examples and this repo's benches register:
      (a) no shape field survives in the specialised body as an `a.<field>` token;
      (b) the specialised body IS the generic body with exactly those tokens replaced by the literals its own header names -- an
          independent regex substitution with identifier boundaries reproduces it byte for byte, so nothing landed inside a
          longer identifier and nothing else changed;
      (c) generic and specialised text both build for gfx950."""
    w = _worlds_incl_schemas()[name]()
    gen = w.generated_kernel_source(compile=True)
    spec = w.generated_kernel_source(compile=True, steady=True)
    k = 'extern "C" __global__'
    gbody, sbody = gen[gen.index(k):], spec[spec.index(k):]
    # (a)
    left = set(re.findall(r"(?<![\w.])a\.(\w+)", sbody))
    assert not left & (set(SHAPE_SCALARS) | set(SHAPE_ARRAYS)), left & (set(SHAPE_SCALARS) | set(SHAPE_ARRAYS))
    assert {"src", "live", "save_dst", "save_frame", "dt_bits", "len", "parts", "part_stride", "n_units", "ff_rows", "ff_blocks"} <= left, left
    # (b) the literals, as the specialised text's own header line states them
    m = re.search(r"// specialised: (\d+) ops \(bits ([0-9a-f]+)\), (\d+) Saves, rows ([0-9a-f]+) / live ([0-9a-f]+) / load ([0-9a-f]+), masks ([0-9a-f]+) / ([0-9a-f]+), nt (\d+), cached ([0-9a-f]+), nt loads (\d+), roles of (\d+), live block (written|left unwritten), value tags (\d)", spec)
    n_ops, op_bits, n_saves, rows, live, load, pm, lpm, nt, cached, ntl, dps = (int(m.group(i), 16 if i in (2, 4, 5, 6, 7, 8, 10) else 10) for i in range(1, 13))
    assert n_ops == 2 * n_saves + 1 and op_bits == sum(1 << (2 * k) for k in range(n_saves + 1)), "the steady SyncTest tick: Advance, (Save, Advance) x D"
    lit = {"op_bits": f"0x{op_bits:x}ull", "n_ops": f"{n_ops}u", "n_saves": f"{n_saves}u", "n_steps": f"{bin(op_bits).count('1')}u", "src_is_live": "0u", "skip_live": "1u" if m.group(13) == "left unwritten" else "0u", "dp_s": f"{dps}u",
           "nt": f"{nt}u", "cached_saves": f"{cached}u", "live_rows": f"0x{live:x}ull", "load_rows": f"0x{load:x}ull", "live_pmask": f"{lpm}u", "nt_loads": f"{ntl}u",
           "vtags": f"{m.group(14)}u", "mtab": "((const unsigned char*)0)"}                      # a specialised copy serves plain launches only: no member records
    want = gbody
    want = re.sub(r"(?<![\w.])a\.save_rows\[si\]", f"0x{rows:x}ull", want)
    want = re.sub(r"(?<![\w.])a\.save_pmask\[si\]", f"{pm}u", want)
    for f in SHAPE_SCALARS:
        want = re.sub(r"(?<![\w.])a\." + f + r"(?!\w)", lit[f], want)
    want = want.replace(f"    for (uint32_t op = 0; op < {n_ops}u; ++op) {{", f"#pragma unroll\n    for (uint32_t op = 0; op < {n_ops}u; ++op) {{", 1)
    assert sbody == want


def test_specialiser_token_rule_on_text_no_generator_emits_yet():
    """The library's own replace (kernel_gen.hpp jit_replace_token, reached through the ggrs_dbg_replace_token test hook): a field is
    rewritten only as a whole `a.<name>` token -- not inside a longer identifier, not as the member of another object."""
    import ctypes as C
    from bevy_ggrs_amd import _ffi
    lib = C.CDLL(_ffi.LIB_PATH)
    lib.ggrs_dbg_replace_token.restype = C.c_int
    lib.ggrs_dbg_replace_token.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64]

    def rep(body, tok, val):
        out = C.create_string_buffer(4096)
        n = lib.ggrs_dbg_replace_token(body.encode(), tok.encode(), val.encode(), out, 4096)
        return n, out.value.decode()
    probe = "a.nt a.nt_x xa.nt s.a.nt a.n_saves2 (a.n_saves) a.nt;a.nt+a.nt a.save_rows[si] a.save_rowsX[si] a.save_rows[sj] a.nt"
    assert rep(probe, "a.nt", "1u") == (5, "1u a.nt_x xa.nt s.a.nt a.n_saves2 (a.n_saves) 1u;1u+1u a.save_rows[si] a.save_rowsX[si] a.save_rows[sj] 1u")
    assert rep(probe, "a.n_saves", "8u") == (1, probe.replace("(a.n_saves)", "(8u)"))
    assert rep(probe, "a.save_rows[si]", "0x7full") == (1, probe.replace(" a.save_rows[si] ", " 0x7full "))
    assert rep("a.nt", "a.nt", "a.nt") == (1, "a.nt")                    # a value that contains the token does not loop
    assert rep("", "a.nt", "1u") == (0, "")


def test_generated_kernel_unrolls_this_worlds_schema():
    src = particles().generated_kernel_source()
    body = src[src.index('#line 1 "ggrs_jit_tick"'):]
    assert len(re.findall(r"#define o\d+\(blk\)", body)) == 14          # Transform 10 + Velocity 3 + Ttl 1 word columns
    assert body.count("SeaStream st;") == 0 and "mt0" in body and "mt1" in body  # checksum_component x 2 (Velocity, Transform.translation): 12 hashed bytes each -> the spelled-out form with a memoised 4-byte tail
    assert "0xc3480000u" in body                                         # gravity.y = -200.0 as exact bits
    assert "PARTICLES_SPAWN" not in body and body.count("particles.rs:272-280") == 1
    assert "a.spawn_payload[sj]" in body and "particles.rs:258-270" in body              # the spawn system runs inside the group's launch


def test_generator_limits_and_errors():
    w = dry()
    for k in range(5): w.register_component(f"Big{k}", 4, 14)                          # 70 four-byte words per entity > 64
    w.add_system(bg.SYS_ADD_U32, comp=(0,), word=(0,), iparam=(1,))
    with pytest.raises(bg.GgrsHipError) as ei:
        w.generated_kernel_source()
    assert ei.value.code == bg.GGRS_E_INVALID and "does not cover" in str(ei.value)

    w = dry()
    A = w.register_component("A", 4, 1); K = w.register_component("K", 4, 1, rollback=False)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(1) += 1; }", [(A, 0), (K, 0)])
    with pytest.raises(bg.GgrsHipError):                                   # may WRITE a live-only word: not replayable, stays per-request
        w.generated_kernel_source()

    w = dry()
    A = w.register_component("A", 4, 1)
    with pytest.raises(bg.GgrsHipError) as ei:                             # a user's compile error surfaces at registration, GPU or not
        w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) += nope; }", [(A, 0)], name="broken")
    assert "broken" in str(ei.value) and "nope" in str(ei.value)


def _eight_byte_words(n_words):
    w = dry(400)
    for k in range(0, n_words, 8): w.register_component(f"Wide{k}", 8, min(8, n_words - k))      # two four-byte register units per word
    w.add_system(bg.SYS_TTL_DESPAWN, comp=(0,), word=(0,))
    return w


def _four_byte_words(n_words):
    w = dry(400)
    for k in range(0, n_words, 13): w.register_component(f"Thin{k}", 4, min(13, n_words - k))
    w.add_system(bg.SYS_ADD_U32, comp=(0,), word=(0,), iparam=(1,))
    return w


def _builtin_on_live_only():
    w = dry(400)
    w.register_component("A", 4, 1); K = w.register_component("K", 4, 1, rollback=False)
    w.add_system(bg.SYS_ADD_U32, comp=(K,), word=(0,), iparam=(1,))
    return w


def _checksummed_live_only():
    w = dry(400)
    A = w.register_component("A", 4, 1); K = w.register_component("K", 4, 1, rollback=False)
    w.checksum_component(K, [0])
    w.add_system(bg.SYS_ADD_U32, comp=(A,), word=(0,), iparam=(1,))
    return w


@pytest.mark.parametrize("make,covered", [pytest.param(lambda: _eight_byte_words(64), True, id="units_at_the_limit"), pytest.param(lambda: _four_byte_words(65), False, id="words_over_the_limit"),
                                          pytest.param(_builtin_on_live_only, False, id="builtin_system_on_live_only"), pytest.param(_checksummed_live_only, False, id="checksummed_live_only")])
def test_generator_refuses_before_it_writes(make, covered):
    """What the generator does not cover is refused as a whole, with the one message of ggrs_hip_generated_kernel_source; 128 four-byte units (JIT_MAX_UNITS) still generate."""
    w = make()
    if covered:
        src = w.generated_kernel_source()
        assert len(re.findall(r"#define o\d+\(blk\)", src)) == 64 and "#error" not in src
        return
    with pytest.raises(bg.GgrsHipError) as ei:
        w.generated_kernel_source()
    assert ei.value.code == bg.GGRS_E_INVALID
    assert "the kernel generator does not cover this world (a system writes a live-only component, or more than 128 four-byte units / 64 words per entity)" in str(ei.value)


def test_layout_only_world_has_no_device_behind_it():
    w = particles()
    with pytest.raises(bg.GgrsHipError) as ei:
        w.spawn(1, {0: None, 1: None, 2: None})
    assert ei.value.code == bg.GGRS_E_NO_DEVICE
    with pytest.raises(bg.GgrsHipError):
        w.handle_requests([bg.SaveGameState(0)])


def test_static_and_generated_kernels_share_one_device_text():
    """kernels.hpp includes device_prelude.hpp as code, kernel_gen.hpp includes it as a string for hiprtc: no second copy of
    the SeaHash constants or the box_game arithmetic anywhere in csrc/."""
    csrc = os.path.join(ROOT, "bevy_ggrs_amd", "csrc")
    k = open(os.path.join(csrc, "kernels.hpp")).read()
    h = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.startswith(("host_", "kernel_gen", "ggrs_hip")))
    p = open(os.path.join(csrc, "device_prelude.hpp")).read()
    assert '#include "device_prelude.hpp"' in k and '#include "device_prelude.hpp"' in h
    assert "0x6eed0e9da4d94a4f" in p and "0x6eed0e9da4d94a4f" not in k and "0x6eed0e9da4d94a4f" not in h
    assert "void box_move_math" in p and "void box_move_math" not in k
    assert not re.search(r"^\s*#", p[p.index("GGRS_SHARED_CODE(\n"):], re.M), "no preprocessor directive inside the macro argument"


def test_narrow_words_and_custom_hashers_generate():
    """1- and 2-byte words (bool / u8 enum / u16 fields) and a user-written checksum hasher: the generator emits typed narrow
    accesses and inlines the hasher; the text builds for gfx950."""
    w = dry()
    T, V, L = cm.build_particles(w, schema="full")[:3]
    F = w.register_component("Flags", 2, 2)
    w.checksum_component(F, [1, 0])
    w.checksum_component(3 + 1, [0])                                    # Visibility: one byte through the hasher
    w.checksum_component_custom(T, "__device__ ggrs_u64 ggrs_hash(const GgrsComponent& c) { GgrsHasher h; h.write_u32(c.u32(0)); h.write_u32(c.u32(1)); h.write_u32(c.u32(2)); return h.finish(); }")
    for steady in (False, True):
        src = w.generated_kernel_source(compile=True, steady=steady)
        assert "GGRS_G uint8_t*" in src and "GGRS_G uint16_t*" in src and "ggrs_hash_0::ggrs_hash(cv)" in src
        assert re.search(r"st\.write\(w\d+_0, 1u\)", src) and re.search(r"st\.write\(w\d+_0, 2u\)", src)


# ---- register / scratch budget of the kernels the library writes (static: hiprtc cross-compiles, the code object's metadata says what the
# kernel needs).  The generated kernel is HBM-bound and hides latency with occupancy: 8 waves per SIMD need <= 64 VGPRs, and a spill to
# scratch would add HBM traffic of its own.  VGPRs of the tile role when this test was written (steady / generic): headline 28 / 43, allhot 38 / 47, full 28 / 63 (the
# steady copy of the full schema does not even load the rows no system writes); the fold-forward role (round 5) keeps 4 eight-byte loads in flight per lane so that it
# stays below the tile role's need (with 16 the headline's steady copy went from 28 to 41 VGPRs and its launch from 48.9 to 50.1 us).
def _resources(src: str) -> dict:
    import ctypes as C, subprocess, tempfile
    rtc = C.CDLL("libhiprtc.so")
    opts = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]
    prog = C.c_void_p()
    assert rtc.hiprtcCreateProgram(C.byref(prog), src.encode(), b"k.hip", 0, None, None) == 0
    arr = (C.c_char_p * len(opts))(*opts)
    assert rtc.hiprtcCompileProgram(prog, len(opts), arr) == 0
    n = C.c_size_t(); rtc.hiprtcGetCodeSize(prog, C.byref(n)); code = C.create_string_buffer(n.value); rtc.hiprtcGetCode(prog, code)
    with tempfile.NamedTemporaryFile(suffix=".hsaco") as f:
        f.write(code.raw); f.flush()
        notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
    return {k: int(re.search(re.escape(k) + r":\s*(\d+)", notes)[1]) for k in (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="no llvm-readelf")
@pytest.mark.parametrize("schema,n,steady_vgprs", [("headline", 1_000_000, 32), ("allhot", 1_000_000, 48), ("full", 1_000_000, 64), ("headline", 4_000_000, 48)])
def test_generated_kernels_keep_their_register_budget(schema, n, steady_vgprs):
    """(the headline at 4 M keeps VALUE TAGS -- its steady Save is bound by bytes --: the steady copies stay within 8 waves per SIMD without a
    spill; the GENERIC kernel of such a world, which serves its first 16 ticks and odd shapes only, may park wave-uniform values in VGPR lanes (SGPR spills:
    no memory traffic) but never in scratch.)"""
    w = dry(n, 9)
    cm.build_particles(w, schema=schema)
    tags = "value tags 1" in w.generated_kernel_source(steady=True)
    assert tags == ((schema, n) in (("headline", 4_000_000),))
    for steady, limit in ((True, steady_vgprs), (False, 64)):
        r = _resources(w.generated_kernel_source(steady=steady))
        assert r[".private_segment_fixed_size"] == 0 and r[".vgpr_spill_count"] == 0, (schema, steady, r)
        assert r[".sgpr_spill_count"] == 0 or (tags and not steady), (schema, steady, r)
        assert r[".vgpr_count"] <= limit, (schema, steady, r)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")
def test_device_spawn_kernel_meets_without_cache_wide_operations_and_stays_resident():
    """A world whose systems spawn on the device runs as ONE resident launch (its capacity is bounded by what the device holds of the kernel) whose workgroups meet
    through {epoch, value} mailbox words.  Static checks of that kernel: 80 VGPRs at most (6 workgroups per CU) and no scratch; no agent-scope release / acquire anywhere
    (`buffer_wbl2` / `buffer_inv`: a writeback / an invalidate of a whole L2 each -- with an acquire inside the poll loop a rendezvous cost ~100 us,
    profiles/r06z/device_spawn_session.txt against profiles/r06m); the mailbox words, the children's links and the parents' records go through as sc1."""
    import ctypes as C, subprocess, tempfile
    import test_gpu_device_spawn as t
    w = dry(280_256, 9)
    cell = w.register_component("Cell", 4, 4)
    w.checksum_component(cell, [0, 1, 2, 3])
    w.add_custom_system(t.SPLIT_SRC, [(cell, 0), (cell, 1), (cell, 2), (cell, 3)], iparam=(1,), name="split")
    w.add_spawn_system(t.CHILD_SRC, [cell], [(cell, 0), (cell, 1), (cell, 2), (cell, 3)], payload_stride=t.PARENT, name="child")
    src = w.generated_kernel_source()
    assert "sp_post(" in src and "sp_await(" in src and "__threadfence" not in src.split("extern \"C\" __global__")[1]
    r = _resources(src)
    assert r[".vgpr_count"] <= 80 and r[".private_segment_fixed_size"] == 0 and r[".vgpr_spill_count"] == 0, r
    rtc = C.CDLL("libhiprtc.so")
    opts = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]
    prog = C.c_void_p()
    assert rtc.hiprtcCreateProgram(C.byref(prog), src.encode(), b"k.hip", 0, None, None) == 0
    assert rtc.hiprtcCompileProgram(prog, len(opts), (C.c_char_p * len(opts))(*opts)) == 0
    n = C.c_size_t(); rtc.hiprtcGetCodeSize(prog, C.byref(n)); code = C.create_string_buffer(n.value); rtc.hiprtcGetCode(prog, code)
    with tempfile.NamedTemporaryFile(suffix=".hsaco") as f:
        f.write(code.raw); f.flush()
        asm = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", f.name], capture_output=True, text=True, check=True).stdout
    assert "buffer_wbl2" not in asm and "buffer_inv" not in asm
    sc1 = [ln for ln in asm.splitlines() if " sc1" in ln]
    assert sum("global_store" in ln for ln in sc1) >= 12 and sum("global_load" in ln for ln in sc1) >= 12, len(sc1)


_SCC_WRITERS = re.compile(r"\bs_(and|or|xor|andn2|orn2|nand|nor|xnor|add|sub|addc|subb|lshl|lshr|ashr|bfe|bfm|not|wqm|bcnt[01]|min|max|abs|absdiff|cmp_\w+|bitcmp[01]|and_saveexec|or_saveexec|andn2_saveexec)_?[a-z0-9_]*\b")


def test_inline_asm_that_runs_an_scc_writing_instruction_says_so():
    """set_lanes / store_lanes narrow `exec` with `s_and_b64` inside one asm statement.  `s_and_b64` writes SCC; an asm statement that does not list "scc" among its
    clobbers lets the compiler keep a condition in SCC across it.  It did: with the group's masks as literals (kernel_gen.hpp jit_specialise) `s_bitcmp1_b32` was
    scheduled before store_lanes and the `s_cselect_b64` reading it behind -- a Save's "this column is already there" then followed the exec mask instead of the tags, and
    three seeds of the value-tag fuzz differed from the oracle once every shape was specialised at first sight (profiles/r06ee, r06ff: `live_rows` left a run-time read
    made it pass -- another schedule).  Every asm statement of the generated text is checked, whatever world it is for."""
    w = dry(4_000_000, 9)
    cm.build_particles(w, schema="headline")
    src = w.generated_kernel_source(steady=True)
    assert "value tags 1" in src and "set_lanes(" in src and "store_lanes(" in src
    n = 0
    for m in re.finditer(r'asm volatile\("((?:[^"\\]|\\.)*)"((?:[^;"]|"(?:[^"\\]|\\.)*")*)\);', src):
        text, rest = m.group(1).replace("\\n", " ").replace("\\t", " "), m.group(2)
        if _SCC_WRITERS.search(text):
            n += 1
            assert '"scc"' in rest.rsplit(":", 1)[-1], f"an asm statement runs an SCC-writing instruction without the clobber: {m.group(0)[:200]}"
    assert n == 2, "set_lanes and store_lanes"


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")
@pytest.mark.parametrize("schema,n", [("headline", 4_000_000), ("allhot", 2_000_000), ("full", 4_000_000)])
def test_no_condition_is_carried_in_scc_across_the_exec_narrowing_asm(schema, n):
    """The same on the ISA of a value-tag kernel (the 4 M headline world's steady tick and its generic kernel): between the `s_and_b64 exec, exec, ..` of
    set_lanes / store_lanes and the next instruction that READS SCC there is one that writes it."""
    import ctypes as C, subprocess, tempfile
    w = dry(n, 9)
    cm.build_particles(w, schema=schema)
    assert "value tags 1" in w.generated_kernel_source(steady=True), "a tag-keeping world"
    rtc = C.CDLL("libhiprtc.so")
    readers = re.compile(r"\bs_(cselect_b(32|64)|cbranch_scc[01]|addc_u32|subb_u32|cmov_b(32|64))\b")
    for steady in (True, False):
        src = w.generated_kernel_source(steady=steady)
        opts = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]
        prog = C.c_void_p()
        assert rtc.hiprtcCreateProgram(C.byref(prog), src.encode(), b"k.hip", 0, None, None) == 0
        assert rtc.hiprtcCompileProgram(prog, len(opts), (C.c_char_p * len(opts))(*opts)) == 0
        n = C.c_size_t(); rtc.hiprtcGetCodeSize(prog, C.byref(n)); code = C.create_string_buffer(n.value); rtc.hiprtcGetCode(prog, code)
        with tempfile.NamedTemporaryFile(suffix=".hsaco") as f:
            f.write(code.raw); f.flush()
            isa = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", f.name], capture_output=True, text=True, check=True).stdout
        lines = [l.split("//")[0].strip() for l in isa.splitlines()]
        seen = 0
        for i, l in enumerate(lines):
            if not l.startswith("s_and_b64 exec, exec, s["): continue
            seen += 1
            for later in lines[i + 1:i + 400]:
                if readers.search(later): raise AssertionError(f"steady={steady}: `{later}` reads the SCC that `{l}` (line {i}) left behind")
                if _SCC_WRITERS.search(later) or later.startswith(("s_branch", "s_cbranch", "s_endpgm", "s_setpc")): break
        assert seen >= 2, (steady, seen)
