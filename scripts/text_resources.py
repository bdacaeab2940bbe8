#!/usr/bin/env python3
"""Resource table of dumped kernel texts (scripts/dump_kernel_texts.py): every *.hip of a directory is compiled for gfx950 with hiprtc under the
library's options -- no GPU --, and its registers, scratch, vector-instruction lines and the compiler's "loop not unrolled" diagnostic are
recorded.  Usage: text_resources.py DIR OUT.json [BEFORE.json]   (with BEFORE.json: also prints the before/after table in markdown)"""
import ctypes as C
import json
import multiprocessing as mp
import os
import re
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
OPTS = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]
MULS = ("v_mad_u64_u32", "v_mul_lo_u32", "v_add3_u32")


def compile_text(path):
    rtc = C.CDLL("libhiprtc.so")
    prog = C.c_void_p()
    assert rtc.hiprtcCreateProgram(C.byref(prog), open(path).read().encode(), b"k.hip", 0, None, None) == 0
    rc = rtc.hiprtcCompileProgram(prog, len(OPTS), (C.c_char_p * len(OPTS))(*OPTS))
    n = C.c_size_t(); rtc.hiprtcGetProgramLogSize(prog, C.byref(n)); log = C.create_string_buffer(max(n.value, 1)); rtc.hiprtcGetProgramLog(prog, log)
    assert rc == 0, (path, log.value.decode(errors="replace")[-2000:])
    rtc.hiprtcGetCodeSize(prog, C.byref(n)); code = C.create_string_buffer(n.value); rtc.hiprtcGetCode(prog, code)
    with tempfile.NamedTemporaryFile(suffix=".hsaco") as f:
        f.write(code.raw); f.flush()
        dis = subprocess.run([OBJDUMP, "-d", f.name], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
    lines = [l.split("//")[0].strip() for l in dis.splitlines()]
    r = {k[1:]: int(re.search(re.escape(k) + r":\s*(\d+)", notes)[1]) for k in (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")}
    r["v_lines"] = sum(1 for l in lines if l.startswith("v_"))
    for m in MULS: r[m] = sum(1 for l in lines if l.startswith(m))
    r["not_unrolled"] = "loop not unrolled" in log.value.decode(errors="replace")
    r["plain"] = not open(path).read().startswith("#define GGRS_SPEC")            # kernel_gen.hpp kJitSeaSpelling: specialised copies take the three-mad multiply
    return os.path.basename(path)[:-4], r


if __name__ == "__main__":
    d, out = sys.argv[1], sys.argv[2]
    files = sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(".hip"))
    with mp.Pool(min(8, os.cpu_count() or 1)) as pool:
        table = dict(pool.map(compile_text, files))
    json.dump(table, open(out, "w"), indent=1, sort_keys=True)
    print(f"{len(table)} texts -> {out}; not unrolled: {[k for k, r in table.items() if r['not_unrolled']]}")
    if len(sys.argv) > 3:
        before = json.load(open(sys.argv[3]))
        print("| text | VGPRs | SGPRs | scratch | `v_` lines | `v_mul_lo_u32` | spelling |\n|---|---|---|---|---|---|---|")
        for k in sorted(table):
            b, a = before[k], table[k]
            print(f"| {k} | {b['vgpr_count']} → {a['vgpr_count']} | {b['sgpr_count']} → {a['sgpr_count']} | {b['private_segment_fixed_size']} → {a['private_segment_fixed_size']} | "
                  f"{b['v_lines']} → {a['v_lines']} | {b['v_mul_lo_u32']} → {a['v_mul_lo_u32']} | {'plain' if a['plain'] else 'three mads'} |")
