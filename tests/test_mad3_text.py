"""The headline world's steady kernel with the three-mad SeaHash multiply (csrc/device_prelude.hpp sea_mul_p_mad3, chosen per text by
csrc/kernel_gen.hpp kJitSeaSpelling), checked WITHOUT a GPU: the text goes through hiprtc for gfx950 under the library's options, as
tests/test_valu_trim_text.py compiles it, and this module reads the compiler's log as well as the code."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

import test_valu_trim_text as vt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# v_mul_lo_u32 instructions of the parent commit's (8602611) headline steady copy, obtained by running `_count(vt._compile(vt._steady_text())[0], "v_mul_lo_u32")`
# -- this module's helper, same process set-up, same hiprtc, same options -- on that commit's library
PARENT_MUL_LO = 309


def _count(lines, op):
    return sum(1 for l in lines if l.startswith(op))


def _hiprtc_log(src):
    """the compiler's diagnostics for the text (warnings included: the compile itself succeeds)"""
    rtc = C.CDLL("libhiprtc.so")
    opts = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]
    prog = C.c_void_p()
    assert rtc.hiprtcCreateProgram(C.byref(prog), src.encode(), b"k.hip", 0, None, None) == 0
    rc = rtc.hiprtcCompileProgram(prog, len(opts), (C.c_char_p * len(opts))(*opts))
    n = C.c_size_t(); assert rtc.hiprtcGetProgramLogSize(prog, C.byref(n)) == 0
    log = C.create_string_buffer(max(n.value, 1)); assert rtc.hiprtcGetProgramLog(prog, log) == 0
    rtc.hiprtcDestroyProgram(C.byref(prog))
    assert rc == 0, log.value.decode(errors="replace")[-3000:]
    return log.value.decode(errors="replace")


@pytest.fixture(scope="module")
def text():
    return vt._steady_text()


@pytest.fixture(scope="module")
def steady(text):
    return vt._compile(text)


def test_the_op_loop_is_unrolled_and_the_compiler_says_nothing_else(text):
    """`#pragma unroll` without a count is silently dropped once the body is large enough: the copy would walk the op list in a rolled loop (418 vector
    instructions, 46 VGPRs).  The loop head a specialised copy compiles carries the trip count (kernel_gen.hpp save_arm)."""
    assert "#else\n#pragma unroll 17u\n    for (uint32_t op = 0; op < 17u; ++op) {\n#endif\n" in text and text.startswith("#define GGRS_SPEC 1\n")      # Load, then 8 x (Advance, Save): the steady SyncTest tick at depth 8
    log = _hiprtc_log(text)
    assert "loop not unrolled" not in log, log[-3000:]


@vt.needs_tools
def test_every_save_of_the_unrolled_loop_folds_per_lane(steady):
    lines, _ = steady
    assert _count(lines, "ds_xor_b64") >= 16, "8 Saves x 2 checksummed components, folded per lane in LDS"


@vt.needs_tools
def test_the_hot_multiplies_are_v_mad_u64_u32(steady):
    lines, _ = steady
    n, mads = _count(lines, "v_mul_lo_u32"), _count(lines, "v_mad_u64_u32")
    print(f"v_mul_lo_u32: {n} (parent {PARENT_MUL_LO}), v_mad_u64_u32: {mads}")
    assert n < 0.25 * PARENT_MUL_LO, (n, PARENT_MUL_LO)
    assert mads >= 3 * 2 * 4 * 2 * 8, mads                 # 3 per multiply, 2 multiplies per diffuse, 4 hot diffuses per checksummed component, 2 components, 8 Saves


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_the_host_build_of_the_prelude_compiles_and_keeps_the_plain_multiply():
    """The register constraint of the multiply ("v") means nothing to the host compiler: it sits under __HIP_DEVICE_COMPILE__, and the host's hot diffuse is
    spelled x * SEA_P.  -fsyntax-only over a translation unit that includes the prelude as the library's host code does."""
    tu = ('#include <hip/hip_runtime.h>\n#include <cstdint>\n#define GGRS_SHARED_CODE(...) __VA_ARGS__\n#include "%s"\n'
          'static_assert(sizeof(GGRS_VGPR_OPAQUE(0), 0) == sizeof(int), "nothing on the host");\n'
          'uint64_t f(uint64_t x) { return sea_pair_folded(sea_order_lane_folded(x), sea_inner_folded(x, sea_tail_folded(1u, 12))); }\n'
          'uint64_t g(uint64_t x) { return GGRS_SEA_MUL_HOT(x); }\n' % os.path.join(ROOT, "bevy_ggrs_amd", "csrc", "device_prelude.hpp"))
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "prelude_host.cpp")
        open(p, "w").write(tu)
        cc = HIPCC if os.path.exists(HIPCC) else "hipcc"
        r = subprocess.run([cc, "--offload-host-only", "-std=c++17", "-Wall", "-fsyntax-only", "-x", "hip", p], capture_output=True, text=True)
        assert r.returncode == 0 and "prelude" not in r.stderr, r.stderr[-3000:]        # no error, and no warning that names either file
        pre = subprocess.run([cc, "--offload-host-only", "-std=c++17", "-E", "-x", "hip", p], capture_output=True, text=True, check=True).stdout
        assert "uint64_t g(uint64_t x) { return ((x) * SEA_P); }" in pre, pre[-600:]
