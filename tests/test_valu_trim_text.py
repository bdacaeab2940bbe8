"""The headline world's steady kernel after the vector-ALU trims (csrc/kernel_gen.hpp), checked WITHOUT a GPU: its text is compiled for gfx950 with
hiprtc under the library's options (as tests/test_generated_kernel.py _resources does), disassembled, and its vector instructions are counted.
The launch is bound by its vector ALUs, so the static count is what the trims are about."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import bevy_ggrs_amd as bg
import common as cm

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

# `_valu_count(_steady_text())` of the parent commit (23bf89c, before the trims), obtained by running THIS helper -- same process set-up, same hiprtc,
# same options -- on that commit's library
PARENT_VALU = 1625


def _steady_text():
    w = bg.World(1_000_000, max_depth=9, flags=bg.GGRS_WORLD_LAYOUT_ONLY)
    cm.build_particles(w, schema="headline")
    try:
        return w.generated_kernel_source(steady=True)
    finally:
        w.close()


def _compile(src):
    """(disassembly lines, resource notes) of the text's gfx950 code object"""
    rtc = C.CDLL("libhiprtc.so")
    opts = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]
    prog = C.c_void_p()
    assert rtc.hiprtcCreateProgram(C.byref(prog), src.encode(), b"k.hip", 0, None, None) == 0
    arr = (C.c_char_p * len(opts))(*opts)
    assert rtc.hiprtcCompileProgram(prog, len(opts), arr) == 0
    n = C.c_size_t(); rtc.hiprtcGetCodeSize(prog, C.byref(n)); code = C.create_string_buffer(n.value); rtc.hiprtcGetCode(prog, code)
    with tempfile.NamedTemporaryFile(suffix=".hsaco") as f:
        f.write(code.raw); f.flush()
        dis = subprocess.run([OBJDUMP, "-d", f.name], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
    lines = [l.split("//")[0].strip() for l in dis.splitlines()]
    res = {k: int(re.search(re.escape(k) + r":\s*(\d+)", notes)[1]) for k in (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")}
    return [l for l in lines if l], res


def _valu_count(lines):
    return sum(1 for l in lines if l.startswith("v_"))


@pytest.fixture(scope="module")
def steady():
    return _compile(_steady_text())


needs_tools = pytest.mark.skipif(not (os.path.exists(OBJDUMP) and os.path.exists(READELF)), reason="no llvm-objdump / llvm-readelf")


@needs_tools
def test_steady_headline_kernel_holds_at_least_4_percent_fewer_vector_instructions(steady):
    lines, _ = steady
    n = _valu_count(lines)
    print(f"vector instructions: {n} (parent {PARENT_VALU}, {100.0 * (n - PARENT_VALU) / PARENT_VALU:+.1f} %)")
    assert n <= 0.96 * PARENT_VALU, (n, PARENT_VALU)


@needs_tools
def test_liveness_is_not_carried_as_a_0_1_register_that_is_compared_with_1_again(steady):
    """The parent assigned `alive_0 = false` under a divergent branch: the compiler carried the bool as 0/1 in a VGPR (v_cndmask_b32 vN, 0, 1, mask) and turned
    it back into a lane mask with a v_cmp_* against 1 in every section of the unrolled loop.  In the hot loop -- from the first per-lane LDS xor of a Save to the
    last -- no such select's register is read by a vector compare with the constant 1 while it holds that value."""
    lines, _ = steady
    xors = [i for i, l in enumerate(lines) if l.startswith("ds_xor_b64")]
    assert len(xors) >= 16, "8 Saves x 2 checksummed components, folded per lane in LDS"
    hits = _carried_bool_round_trips(lines[xors[0]:xors[-1] + 1])
    assert not hits, hits


def _carried_bool_round_trips(lines):
    """(select, compare) pairs: a `v_cndmask_b32 vN, 0, 1, mask` whose 0/1 value -- as it is, or passed on through selects, ands, ors and moves -- is read by a
    vector compare against the constant 1.  Straight-line approximation over the listing (the hot loop is unrolled)."""
    hits = []
    for i, l in enumerate(lines):
        m = re.match(r"v_cndmask_b32(?:_e64|_e32)? (v\d+), 0, 1,", l)
        if not m: continue
        carry = {m.group(1)}
        for later in lines[i + 1:i + 80]:
            if not later.startswith("v_") or " " not in later: continue
            op, rest = later.split(None, 1)
            ops = [o.strip() for o in rest.split(",")]
            if op.startswith("v_cmp"):
                if carry & set(ops[1:]) and "1" in ops[1:]: hits.append((l, later))
                continue
            passes_on = op.split("_e")[0] in ("v_cndmask_b32", "v_and_b32", "v_or_b32", "v_mov_b32") and carry & set(ops[1:])
            if passes_on: carry.add(ops[0])
            else: carry.discard(ops[0])
            if not carry: break
    return hits


def test_the_round_trip_detector_knows_the_pattern():
    parent = ["v_cndmask_b32_e64 v12, 0, 1, s[14:15]", "v_cndmask_b32_e64 v1, 0, 1, vcc", "v_cndmask_b32_e64 v1, v12, v1, s[26:27]", "v_and_b32_e32 v1, 1, v1",
              "v_cndmask_b32_e64 v21, v13, v15, s[26:27]", "v_cmp_eq_u32_e64 s[14:15], 1, v1", "s_waitcnt lgkmcnt(0)", "v_cmp_ne_u32_e64 s[22:23], 0, v1"]
    assert len(_carried_bool_round_trips(parent)) == 2             # both selects reach the compare
    assert not _carried_bool_round_trips(["v_cndmask_b32_e64 v16, 0, 1, s[18:19]", "v_cmp_ne_u32_e64 s[22:23], 0, v16", "v_mov_b32_e32 v16, 0", "v_cmp_eq_u32_e32 vcc, 1, v16"])


@needs_tools
def test_steady_headline_kernel_keeps_its_register_budget(steady):
    _, r = steady
    assert r[".vgpr_count"] <= 32, r
    assert r[".private_segment_fixed_size"] == 0 and r[".vgpr_spill_count"] == 0 and r[".sgpr_spill_count"] == 0, r
