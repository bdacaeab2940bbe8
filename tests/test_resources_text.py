"""Device-resident rollback resources (ggrs_hip_register_resource, _checksum_resource, _add_resource_system, _add_custom_system_resources, _resource_read / _write),
checked WITHOUT a GPU on GGRS_WORLD_LAYOUT_ONLY worlds: the entry points exist in every layer that mirrors the ABI; with no resource binding the new entry point gives
the commands entry point's text byte for byte; a world without resources names none of the new identifiers; every refusal of include/ggrs_hip.h answers
GGRS_E_INVALID with a message naming the resource or the system; the clock world's generated text keeps the resource words in wave-uniform registers, compiles for
gfx950 and needs no scratch; a resource system that writes through a word it did not bind does not compile."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import bevy_ggrs_amd as bg
import common as cm
from bevy_ggrs_amd import _ffi
from resources_common import BEFORE_SRC, TICK_SRC, build_clock, register_clock_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]
NOP = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) += 1u; }"
RNOP = "__device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame&) { r.u32(0) += 1u; }"
NEW_IDENTIFIERS = ("res_src", "res_alt", "GgrsResources", "res_u32", "ent.rs_[", " rs_ = ", "ggrs_res_sys_", "rr_.w[", "rp_ ^= ")


def layout_world(cap=600, flags=0):
    return bg.World(cap, max_depth=8, flags=bg.GGRS_WORLD_LAYOUT_ONLY | flags)


def _one(w):
    H = w.register_component("Hp", 4, 1); w.checksum_component(H, [0])
    return H


def _refused(w, *needles):
    with pytest.raises(bg.GgrsHipError) as e:
        w.generated_kernel_source()
    assert e.value.code == bg.GGRS_E_INVALID, str(e.value)
    for n in needles: assert n in str(e.value), (n, str(e.value))


def _invalid(call, *needles):
    with pytest.raises(bg.GgrsHipError) as e:
        call()
    assert e.value.code == bg.GGRS_E_INVALID, str(e.value)
    for n in needles: assert n in str(e.value), (n, str(e.value))


def test_entry_points_exist_in_header_library_ctypes_mirror_and_rust_shim():
    hdr = open(os.path.join(ROOT, "include", "ggrs_hip.h")).read()
    rs = open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "bevy_ggrs_hip.hpp")).read()
    lib = C.CDLL(_ffi.LIB_PATH)
    for fn in ("ggrs_hip_register_resource", "ggrs_hip_checksum_resource", "ggrs_hip_add_resource_system", "ggrs_hip_add_custom_system_resources", "ggrs_hip_resource_read",
               "ggrs_hip_resource_write"):
        assert re.search(r"\bint %s\(ggrs_world\* w," % fn, hdr), fn
        assert hasattr(lib, fn) and fn in _ffi.SIGNATURES and ("pub fn %s(w: *mut ggrs_world," % fn) in rs and (fn + "(w, ") in hpp, fn
    assert re.search(r"int ggrs_hip_register_resource\(ggrs_world\* w, const char\* name, uint32_t word_bytes, uint32_t n_words,\s*const void\* init_words, uint32_t\* res_id_out\);", hdr)
    assert re.search(r"const ggrs_command_binding\* cmds, uint32_t n_cmds,\s*const ggrs_resource_binding\* res, uint32_t n_res\);", hdr)
    assert re.search(r"#define GGRS_SYS_RESOURCE\s+9u\b", hdr) and "pub const GGRS_SYS_RESOURCE: u32 = 9;" in rs and bg.SYS_RESOURCE == 9
    assert re.search(r"#define GGRS_RESOURCE_MAX\s+8\b", hdr) and re.search(r"#define GGRS_RESOURCE_MAX_BYTES\s+64\b", hdr) and re.search(r"#define GGRS_RESOURCE_MAX_BINDINGS\s+8\b", hdr)
    assert (bg.RESOURCE_MAX, bg.RESOURCE_MAX_BYTES, bg.RESOURCE_MAX_BINDINGS) == (8, 64, 8)
    assert "#define GGRS_HIP_ABI_VERSION 9" in hdr and _ffi.lib.ggrs_hip_abi_version() == 9
    assert "typedef struct { uint32_t res; uint32_t word; } ggrs_resource_binding;" in hdr and "pub struct ggrs_resource_binding {" in rs and "pub struct ggrs_resource_system_desc {" in rs
    assert C.sizeof(_ffi.ResourceBinding) == 8 and C.sizeof(_ffi.ResourceSystemDesc) == 16 + 4 + 64 + 4 + 16 + 16
    for words in ("__device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame& f);", "runs once per simulated frame, at its registration position",
                  "values, not references", "A resource system registered earlier has already run for this frame, one registered later has", "no registration-order rule",
                  "with n_res == 0 the call behaves exactly as that one", "Every SaveWorld stores the resources with the snapshot and every LoadWorld restores them",
                  "no launch reads resource words from a location it writes", "inserting or removing a resource at run time", "1- and 2-byte words", "a custom resource hasher",
                  "spawn systems with resource bindings", "WRITING or reducing into a resource", "not a kind for ggrs_hip_add_system"):
        assert words in hdr, words


def test_zero_resource_bindings_is_the_commands_entry_point():
    texts = []
    for how in ("commands", "resources"):
        w = layout_world(); H = _one(w)
        d = _ffi.CustomSystemDesc(); d.name, d.source, d.n_bindings = b"custom", NOP.encode(), 1; d.comp[0], d.word[0] = H, 0
        if how == "commands": w._check(w._lib.ggrs_hip_add_custom_system_commands(w._p, C.byref(d), None, 0, None, 0, None, 0))
        else: w._check(w._lib.ggrs_hip_add_custom_system_resources(w._p, C.byref(d), None, 0, None, 0, None, 0, None, 0))
        texts.append(w.generated_kernel_source())
    assert texts[0] == texts[1]
    for ident in NEW_IDENTIFIERS: assert ident not in texts[1], ident


def test_worlds_without_resources_keep_their_text():
    for form, steady in (("generic", False), ("steady", True)):
        w = bg.World(1_000_000, max_depth=9, flags=bg.GGRS_WORLD_LAYOUT_ONLY); cm.build_particles(w)
        src = w.generated_kernel_source(steady=steady)
        assert src == open(os.path.join(ROOT, "docs", "generated", f"headline_{form}.hip")).read(), form
        for ident in NEW_IDENTIFIERS: assert ident not in src, ident
    from commands_common import build_stun
    from peer_effects_common import build_strike
    for build in (build_stun, build_strike):
        w = layout_world(); build(w)
        src = w.generated_kernel_source()
        for ident in NEW_IDENTIFIERS: assert ident not in src, ident
    # the plain comparison world too; the clock world names them all
    w = layout_world(); build_clock(w, plain=True)
    src = w.generated_kernel_source()
    for ident in NEW_IDENTIFIERS: assert ident not in src, ident
    w = layout_world(); build_clock(w)
    src = w.generated_kernel_source()
    for ident in NEW_IDENTIFIERS: assert ident in src, ident


def test_refusals_name_the_resource_or_the_system():
    # a world that keeps RollbackDespawned markers
    w = layout_world(); H = _one(w); w.register_resource("Clock", 4, 2)
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, bg.DESPAWN_ROLLBACK))
    _refused(w, "device resources", "'Clock'", "RollbackDespawned markers")
    # a world that spawns on the device with e.spawn(n)
    w = layout_world(); H = _one(w); w.register_resource("Clock", 4, 2)
    w.add_custom_system("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.spawn(1); }", [(H, 0)], name="splitter")
    w.add_spawn_system("__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64 k, const GgrsFrame&, const unsigned char*) { e.u32(0) = (ggrs_u32)k; }", bundle=(H,), bindings=[(H, 0)],
                       payload_stride=0xFFFFFFFF)
    _refused(w, "device resources", "'Clock'", "spawns on the device", "e.spawn(n)")
    # worlds without the generated kernel
    for flags in (bg.GGRS_WORLD_NO_GROUPS, bg.GGRS_WORLD_UNFUSED):
        w = layout_world(flags=flags); H = _one(w); w.register_resource("Clock", 4, 2)
        w.add_system(bg.SYS_ADD_U32, comp=(H,), word=(0,), iparam=(1,))
        _refused(w, "device resources", "'Clock'", "need the generated request-group kernel")
    # more than the limits
    w = layout_world(); _one(w)
    for k in range(8): w.register_resource(f"R{k}", 4, 1)
    _invalid(lambda: w.register_resource("Ninth", 4, 1), "'Ninth'", "GGRS_RESOURCE_MAX")
    w = layout_world(); _one(w); w.register_resource("Wide", 8, 7)
    _invalid(lambda: w.register_resource("Tail", 4, 3), "'Tail'", "56 bytes already registered", "GGRS_RESOURCE_MAX_BYTES")
    w.register_resource("Fits", 4, 2)
    _invalid(lambda: w.register_resource("Byte", 1, 1), "'Byte'", "word_bytes must be 4 or 8")
    _invalid(lambda: w.register_resource("Short", 2, 1), "'Short'", "word_bytes must be 4 or 8")
    # a binding to an unknown resource or word
    w = layout_world(); H = _one(w); R = w.register_resource("Clock", 4, 2)
    _invalid(lambda: w.add_resource_system(RNOP, [(R + 1, 0)], name="tick"), "'tick'", "binding 0", "resource 1", "not registered")
    _invalid(lambda: w.add_resource_system(RNOP, [(R, 2)], name="tick"), "'tick'", "word 2 of resource 0")
    _invalid(lambda: w.add_custom_system(BEFORE_SRC, [(H, 0)], name="reader", resources=[(R, 5)]), "'reader'", "resource binding 0", "word 5 of resource 0")
    _invalid(lambda: w.add_custom_system(BEFORE_SRC, [(H, 0)], name="reader", resources=[(3, 0)]), "'reader'", "resource 3")
    _invalid(lambda: w.checksum_resource(R, [2]), "'Clock'", "word 2")
    _invalid(lambda: w.checksum_resource(4, [0]), "resource 4")
    d = _ffi.CustomSystemDesc(); d.name, d.source, d.n_bindings = b"many", BEFORE_SRC.encode(), 1; d.comp[0], d.word[0] = H, 0
    rb = (_ffi.ResourceBinding * 9)()
    _invalid(lambda: w._check(w._lib.ggrs_hip_add_custom_system_resources(w._p, C.byref(d), None, 0, None, 0, None, 0, rb, 9)), "'many'", "GGRS_RESOURCE_MAX_BINDINGS")
    # a resource system with no binding; GGRS_SYS_RESOURCE is not a kind for ggrs_hip_add_system
    _invalid(lambda: w.add_resource_system(RNOP, [], name="idle"), "'idle'", "no binding")
    _invalid(lambda: w.add_system(bg.SYS_RESOURCE, comp=(H,), word=(0,)), "does not match")
    # GGRS_MAX_SYSTEMS counts resource systems
    w = layout_world(); H = _one(w); R = w.register_resource("Clock", 4, 2)
    for k in range(16): w.add_resource_system(RNOP, [(R, 0)], name=f"t{k}")
    _invalid(lambda: w.add_resource_system(RNOP, [(R, 0)], name="t16"), "'t16'", "too many systems")


def test_no_generated_kernel_knob_is_refused(monkeypatch):
    monkeypatch.setenv("GGRS_TICK_JIT", "0")
    w = layout_world(); H = _one(w); w.register_resource("Clock", 4, 2)
    w.add_system(bg.SYS_ADD_U32, comp=(H,), word=(0,), iparam=(1,))
    _refused(w, "device resources", "'Clock'", "need the generated request-group kernel", "GGRS_TICK_JIT=0")


def test_clock_world_text_keeps_the_words_in_uniform_registers():
    w = layout_world(); build_clock(w)
    src = w.generated_kernel_source()
    body = src.split('extern "C" __global__')[1]
    # loaded once per launch, ahead of the op loop, through the constant address space from the source block's current cell: Big (8-byte words first), then Clock, Wind
    head = body[:body.index("for (uint32_t op = 0;")]
    assert "const GGRS_K unsigned char* const rs_ = (const GGRS_K unsigned char*)(unsigned long)a.res_src;" in head
    for line in ("uint32_t r0 = *(const GGRS_K uint32_t*)(rs_ + 8u);", "uint32_t r1 = *(const GGRS_K uint32_t*)(rs_ + 12u);", "uint32_t r2 = *(const GGRS_K uint32_t*)(rs_ + 16u);",
                 "uint64_t r3 = *(const GGRS_K uint64_t*)(rs_ + 0u);"):
        assert head.count(line) == 1 and body.count(line) == 1, line
    # the resource system: between the two entity systems, outside any liveness test, what comes back pinned into scalar registers
    i_before, i_tick, i_drift = body.index("ggrs_sys_0::ggrs_system(ent, fr0);"), body.index("ggrs_res_sys_0::ggrs_resource_system(rr_, fr1);"), body.index("ggrs_sys_1::ggrs_system(ent, fr2);")
    assert i_before < i_tick < i_drift
    block = body[body.rindex("// resource system 0", 0, i_tick):i_tick]
    assert "alive_0" not in block and "lane" not in block and "e0" not in block
    assert "r0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)rr_.w[0]);" in body and "r3 = uni64(rr_.w[3]);" in body
    # entity reads: copied in by value in front of the call, nothing written back
    assert "ent.rs_[0] = (ggrs_u64)r0;\n                ggrs_sys_0::ggrs_system(ent, fr0);" in body
    assert "ent.rs_[0] = (ggrs_u64)r2;\n                ent.rs_[1] = (ggrs_u64)r0;\n                ggrs_sys_1::ggrs_system(ent, fr2);" in body
    assert not re.search(r"\br\d = [^;]*ent\.", body)
    # stored by the lane that writes the header, into the other cell when the destination is the source block; the live block likewise; the part by one lane per Save
    assert body.count("== a.src ? a.res_alt : 64u);") == 2
    assert re.search(r"\*reinterpret_cast<Header\*>\(dst\) = h;\n\s*\{ unsigned char\* const rc_ = dst \+", body)
    assert "if (gu == 0 && lane == 0) {                                                // device resources: the live world's" in body
    assert "{ SeaStream st; st.write(r0, 4u); st.write(r1, 4u); rp_ ^= st.finish(); }" in body and "{ SeaStream st; st.write(r3, 8u); rp_ ^= st.finish(); }" in body
    assert "acc[4] = rp_;" in body and "s_acc[16 * 5]" in body and "(row % 5u) == 3u" in body
    # the typedef in front of the system's source: four bindings, the fourth an 8-byte word
    assert "namespace ggrs_res_sys_0 {\ntypedef ::GgrsResourcesT<4u, 0x8u> GgrsResources;\n#line 1" in src
    assert "const unsigned char* res_src;" in src and "ggrs_u32 res_alt;" in src
    assert "s_sleep" not in body and "atomicCAS" not in body


def _build(src):
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
    return res, asm


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")
@pytest.mark.parametrize("steady", [False, True])
def test_clock_world_compiles_for_gfx950_without_scratch(steady):
    """The .vgpr_count of the clock world and of the same world without resources are printed here and recorded in profiles/device_resources/README.md; no bound on
    them is fixed -- only: no scratch and no vector-register spills."""
    out = {}
    for which in ("clock", "plain"):
        w = layout_world(); build_clock(w, plain=which == "plain")
        res, asm = _build(w.generated_kernel_source(steady=steady, compile=True))
        print(which, "steady" if steady else "generic", res)
        assert res.get("private_segment_fixed_size") == 0 and res.get("vgpr_spill_count") == 0, (which, res)      # (a scalar register parked in a vector lane is no scratch)
        assert "scratch_" not in asm, which
        out[which] = res
    readme = open(os.path.join(ROOT, "profiles", "device_resources", "README.md")).read()
    form = "steady" if steady else "generic"
    for which in ("clock", "plain"):
        assert re.search(r"\| %s \| %s \| %d \| %d \|" % (which, form, out[which]["vgpr_count"], out[which]["sgpr_count"]), readme), (which, form, out[which])


def test_a_resource_system_that_writes_through_an_unbound_word_does_not_compile():
    w = layout_world(); _one(w); res = register_clock_resources(w)
    C_, Wn, B = res
    # TICK_SRC names r.u32(0), r.u32(1), r.f32(2), r.u64(3): with three bindings the fourth is not bound
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_resource_system(TICK_SRC, [(C_, 0), (C_, 1), (Wn, 0)], name="tick")
    msg = str(e.value)
    assert e.value.code == bg.GGRS_E_INVALID and "resource system 'tick' does not compile" in msg, msg
    assert "no matching member function for call to 'u64'" in msg and "must be a bound 8-byte resource word" in msg, msg
    # the other width does not compile either: binding 3 is Big's 8-byte word, read here as u32
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_resource_system("__device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame&) { r.u32(3) = 1u; }", [(C_, 0), (C_, 1), (Wn, 0), (B, 0)], name="narrow")
    assert "no matching member function for call to 'u32'" in str(e.value) and "must be a bound 4-byte resource word" in str(e.value)
    # an index that is not a constant
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_resource_system("__device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame& f) { r.u32(f.frame & 1) = 1u; }", [(C_, 0), (C_, 1)], name="dyn")
    assert "no matching member function for call to 'u32'" in str(e.value)
    # the declared bindings compile
    w.add_resource_system(TICK_SRC, [(C_, 0), (C_, 1), (Wn, 0), (B, 0)], name="tick")
