"""The sorted query in the text: its entry points exist in every layer (header, ctypes, ffi.rs, the C++ mirror, the Rust and Python shims); its kernels compile
for gfx950 without scratch; and the peer index's kernels, which it launches as they are, are byte-identical to what they were before it existed."""
import hashlib
import os
import re
import subprocess
import tempfile

import pytest

import bevy_ggrs_amd as bg
from bevy_ggrs_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORT_KERNELS = ("k_sort_rows", "k_sort_rekey", "k_sort_small", "k_sort_emit")
SORT_FIRST = "// ------------------------------------------------------------------ SORTED QUERY (ggrs_hip_query_sorted / ggrs_hip_query_sorted_block)"
SORT_LAST = "// ------------------------------------------------------------------ END OF SORTED QUERY"
IX_RANGE_SHA256 = "83919d4ee58ee6bf96442f454288f00d71d38a1fe26d2f7e9ee2d08dc0a512a0"       # the range tests/test_peer_index_model.py cuts, as of the commit before the sorted query


def read(*parts): return open(os.path.join(ROOT, *parts)).read()


def test_the_entry_points_exist_in_every_layer():
    hdr = re.sub(r"/\*.*?\*/", "", read("include", "ggrs_hip.h"), flags=re.S)
    for fn in ("ggrs_hip_query_sorted", "ggrs_hip_query_sorted_block"):
        assert re.search(r"\bint %s\s*\(" % fn, hdr) and fn in _ffi.SIGNATURES and hasattr(_ffi.lib, fn)
        assert re.search(r"pub fn %s\(" % fn, read("rust", "bevy_ggrs_hip", "src", "ffi.rs"))
        assert fn + "(w, " in read("include", "bevy_ggrs_hip.hpp")
    for name, val in (("GGRS_SORT_MAX_KEYS", "4"), ("GGRS_SORT_U", "0u"), ("GGRS_SORT_I", "1u"), ("GGRS_SORT_F", "2u"), ("GGRS_SORT_DESC", "0x100u")):
        assert re.search(r"#define %s\s+%s\b" % (name, val), hdr), name
    assert "typedef struct { uint32_t comp; uint32_t word; uint32_t kind; } ggrs_sort_key;" in hdr
    assert "typedef struct { ggrs_sort_key keys[GGRS_SORT_MAX_KEYS]; uint32_t n_keys; uint32_t flags; } ggrs_sort_desc;" in hdr
    assert "#define GGRS_HIP_ABI_VERSION 9" in re.sub(r"[ \t]+", " ", hdr) and _ffi.lib.ggrs_hip_abi_version() == 9      # functions and structs are added only
    assert (_ffi.SORT_MAX_KEYS, _ffi.SORT_U, _ffi.SORT_I, _ffi.SORT_F, _ffi.SORT_DESC) == (4, 0, 1, 2, 0x100)
    rs = read("rust", "bevy_ggrs_hip", "src", "ffi.rs")
    for const, val in (("GGRS_SORT_MAX_KEYS: usize", "4"), ("GGRS_SORT_U: u32", "0"), ("GGRS_SORT_I: u32", "1"), ("GGRS_SORT_F: u32", "2"), ("GGRS_SORT_DESC: u32", "0x100")):
        assert f"pub const {const} = {val};" in rs, const
    assert re.search(r"pub struct ggrs_sort_key \{\s*pub comp: u32,\s*pub word: u32,\s*pub kind: u32,\s*\}", rs)
    assert re.search(r"pub struct ggrs_sort_desc \{\s*pub keys: \[ggrs_sort_key; GGRS_SORT_MAX_KEYS\],\s*pub n_keys: u32,\s*pub flags: u32,\s*\}", rs)
    lib_rs = read("rust", "bevy_ggrs_hip", "src", "lib.rs")
    assert "pub unsafe fn query_sorted(" in lib_rs and "ffi::ggrs_hip_query_sorted(self.raw" in lib_rs and "pub fn sort_desc(" in lib_rs
    hpp = read("include", "bevy_ggrs_hip.hpp")
    for m in ("static ggrs_sort_desc sort_desc(", "int query_sorted(", "int query_sorted_block("): assert m in hpp, m
    for m in ("query_sorted", "sort_desc"): assert callable(getattr(bg.World, m))
    for dbg in ("ggrs_dbg_set_sort_form", "ggrs_dbg_sorted_query_launch_us"): assert dbg in _ffi.DEBUG_SIGNATURES and hasattr(_ffi.lib, dbg)


def test_the_kernels_sit_in_their_own_section_behind_the_delta_kernels():
    ker = read("bevy_ggrs_amd", "csrc", "kernels.hpp")
    assert ker.count(SORT_FIRST) == 1 and ker.count(SORT_LAST) == 1
    first, last = ker.index(SORT_FIRST), ker.index(SORT_LAST)
    assert ker.index("void k_delta_match_values(") < first < last
    assert not (ker.index("constexpr uint32_t IX_TPB = 256") < first < ker.index("// THE INBOX (ggrs_hip_add_custom_system_effects"))
    section, rest = ker[first:last], ker[:first] + ker[last:]
    for k in SORT_KERNELS: assert f"void {k}(" in section and k not in rest, k
    code = re.sub(r"//[^\n]*", "", section)
    for banned in ("atomicCAS", "atomicExch", "atomicAdd", "atomicMax", "atomicMin", "__builtin_amdgcn_s_sleep", "asm"): assert banned not in code, banned
    assert "ix_small_pass<false>(" in code and "__threadfence_block();" in code and "__syncthreads();" in code      # the small form: the tile bodies, a fence and a barrier


def test_the_peer_index_kernels_are_what_they_were():
    ker = read("bevy_ggrs_amd", "csrc", "kernels.hpp")
    cut = ker[ker.index("constexpr uint32_t IX_TPB = 256"):ker.index("// THE INBOX (ggrs_hip_add_custom_system_effects")]
    assert hashlib.sha256(cut.encode()).hexdigest() == IX_RANGE_SHA256
    assert "k_sort" not in cut and "SortArgs" not in cut
    host = read("bevy_ggrs_amd", "csrc", "ggrs_hip.hip")
    run = host[host.index("int sort_run("):host.index("//   ggrs_dbg_set_sort_form")]
    for launch in ("(k_ix_hist<false>)", "k_ix_scan,", "(k_ix_scatter<false>)", "k_sort_small,", "k_sort_rows,", "k_sort_rekey,", "k_sort_emit,", "k_query_match,", "k_diff_scan,"):
        assert "hipLaunchKernelGGL(" + launch in run, launch


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf")), reason="no hipcc / llvm-readelf")
def test_the_sort_kernels_compile_without_scratch():
    csrc = os.path.join(ROOT, "bevy_ggrs_amd", "csrc")
    flags = re.search(r"^HIPFLAGS \?= (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).replace("$(ARCH)", "gfx950").split()
    with tempfile.NamedTemporaryFile(suffix=".hsaco") as f:
        r = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-Rpass-analysis=kernel-resource-usage", "--offload-device-only", "--no-gpu-bundle-output", "-c", os.path.join(csrc, "ggrs_hip.hip"), "-o", f.name],
                           check=True, capture_output=True, text=True)
        notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
    # the resource remarks, per kernel
    remarks = {}
    for blk in r.stderr.split("remark: Function Name: ")[1:]:
        name = blk.split()[0]
        kind = next((k for k in SORT_KERNELS if k in name), None)
        if kind: remarks[kind] = {k.strip(): int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", blk)}
    assert set(remarks) == set(SORT_KERNELS), sorted(remarks)
    for k, res in remarks.items():
        print(k, res)
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0 and res["VGPRs"] <= 64 and res["Occupancy"] == 8, (k, res)
    assert remarks["k_sort_small"]["LDS Size"] == 6144 and all(remarks[k]["LDS Size"] == 0 for k in SORT_KERNELS if k != "k_sort_small")
    # ... and what the code object's notes say
    seen = set()
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        kind = next((k for k in SORT_KERNELS if k in name), None)
        if not kind: continue
        res = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size|vgpr_count):\s+(\d+)", blk)}
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0, (name, res)
        seen.add(kind)
    assert seen == set(SORT_KERNELS)
