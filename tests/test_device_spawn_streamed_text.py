"""The STREAMED form of the device-spawn kernel (GGRS_TICK_JIT=2, or a world the device cannot hold as one resident grid), checked WITHOUT a GPU
on a GGRS_WORLD_LAYOUT_ONLY world: its workgroups take their tiles by ticket and number the children by a decoupled look-back over per-step tile
descriptors, so the text has a ticket, a look-back and no XCD remap of blockIdx.x, and no per-parity parent records.  Without the knob the world's text is
the resident form's, unchanged.  Its ISA: no cache-wide writeback / invalidate, every polled word, descriptor and child record through sc1, no scratch."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import bevy_ggrs_amd as bg
from test_gpu_device_spawn import CHILD_SRC, PARENT, SPLIT_SRC, build, oracle_child, oracle_split  # noqa: F401  (names only: no test is imported)

OPTS = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]


def splitting_world(capacity=280_256):
    w = bg.World(capacity, max_depth=9, flags=bg.GGRS_WORLD_LAYOUT_ONLY)
    cell = w.register_component("Cell", 4, 4)
    w.checksum_component(cell, [0, 1, 2, 3])
    w.add_custom_system(SPLIT_SRC, [(cell, 0), (cell, 1), (cell, 2), (cell, 3)], iparam=(1,), name="split")
    w.add_spawn_system(CHILD_SRC, [cell], [(cell, 0), (cell, 1), (cell, 2), (cell, 3)], payload_stride=PARENT, name="child")
    return w


def kernel_body(src):
    return src.split('extern "C" __global__')[1]


def test_streamed_text_takes_tiles_by_ticket_and_looks_back(monkeypatch):
    monkeypatch.setenv("GGRS_TICK_JIT", "2")
    src = splitting_world().generated_kernel_source()
    body = kernel_body(src)
    assert "PROGRESS RULE" in src and "strictly lower ticket" in src
    assert "atomicAdd((unsigned long long*)a.sp_ctl, 1ull) - a.sp_ticket_base" in body and "const uint32_t tile = s_tk;" in body
    assert "look back" in body and "sp_await(dsc_ + (hi_ - 1u - lane)" in body and "sp_await_inc(dsc_ + own_" in body
    assert "blockIdx.x" not in body and "(bx & 7u)" not in body and "g8" not in body
    assert "sp_prec" not in body and "sp_link" not in body and "(sj & 1u)" not in body
    # every access to a word another workgroup reads or writes -- descriptors, record offsets, child records, the pool cursor, the read flags -- is an atomic:
    # a relaxed agent-scope load / store / read-modify-write (sp_post / sp_await* / sp_gate are those), never a plain access
    shared = re.compile(r"\b(dsc_ \+|rof_ \+|r_ \+ 9u|rc_ \+|a\.sp_recs|a\.sp_ctl|a\.sp_desc)")
    for ln in body.splitlines():
        code = ln.split("//")[0]
        if shared.search(code) and "ggrs_u64* const" not in code:
            assert re.search(r"__hip_atomic_(load|store|exchange|fetch_add)\(|sp_post\(|sp_await(_inc)?\(|sp_gate\(|atomicAdd\(", code), ln
    # the grid's last tile waits for every tile's read of the starting len before it rewrites that header
    assert body.count("sp_gate(") == 2 and "GGRS_SP_READ" in body
    # the argument block: the streamed fields, and none of the resident form's mailboxes
    assert re.search(r"ggrs_u64\* sp_desc;", src) and re.search(r"ggrs_u64 sp_ticket_base;", src) and "sp_sums;" not in src


def test_without_the_knob_the_text_is_the_resident_form(monkeypatch):
    monkeypatch.delenv("GGRS_TICK_JIT", raising=False)
    src = splitting_world().generated_kernel_source()
    assert "sp_ticket_base" not in src and "sp_desc" not in src and "PROGRESS RULE" not in src
    assert "const uint32_t tile = (bx & 7u) * g8 + (bx >> 3);" in src and "sp_prec" in src
    monkeypatch.setenv("GGRS_TICK_JIT", "1")
    assert splitting_world().generated_kernel_source() == src


def test_the_knob_leaves_worlds_without_device_spawns_alone(monkeypatch):
    import common as cm
    monkeypatch.delenv("GGRS_TICK_JIT", raising=False)
    w = bg.World(1_000_000, max_depth=9, flags=bg.GGRS_WORLD_LAYOUT_ONLY); cm.build_particles(w, schema="headline")
    before = w.generated_kernel_source(), w.generated_kernel_source(steady=True)
    monkeypatch.setenv("GGRS_TICK_JIT", "2")
    w = bg.World(1_000_000, max_depth=9, flags=bg.GGRS_WORLD_LAYOUT_ONLY); cm.build_particles(w, schema="headline")
    assert (w.generated_kernel_source(), w.generated_kernel_source(steady=True)) == before


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")
def test_streamed_isa_has_no_cache_wide_operations_and_no_scratch(monkeypatch):
    monkeypatch.setenv("GGRS_TICK_JIT", "2")
    src = splitting_world(4_000_256).generated_kernel_source()
    rtc = C.CDLL("libhiprtc.so")
    prog = C.c_void_p()
    assert rtc.hiprtcCreateProgram(C.byref(prog), src.encode(), b"k.hip", 0, None, None) == 0
    assert rtc.hiprtcCompileProgram(prog, len(OPTS), (C.c_char_p * len(OPTS))(*OPTS)) == 0
    n = C.c_size_t(); rtc.hiprtcGetCodeSize(prog, C.byref(n)); code = C.create_string_buffer(n.value); rtc.hiprtcGetCode(prog, code)
    with tempfile.NamedTemporaryFile(suffix=".hsaco") as f:
        f.write(code.raw); f.flush()
        asm = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", f.name], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
    assert "buffer_wbl2" not in asm and "buffer_inv" not in asm
    res = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", notes)}
    assert res.get("private_segment_fixed_size") == 0 and res.get("vgpr_spill_count") == 0, res
    # descriptors / record offsets / record flags polled, record words loaded: sc1 loads; descriptors posted, records written: sc1 stores
    sc1 = [ln for ln in asm.splitlines() if " sc1" in ln]
    assert sum("global_load_dwordx2" in ln for ln in sc1) >= 8 and sum("global_store_dwordx2" in ln for ln in sc1) >= 6, len(sc1)
    # the ticket and the record-pool cursor: device-scope read-modify-writes (one add each; tile 0 starts the cursor over with a swap), no retry loop
    assert asm.count("global_atomic_add_x2") == 2 and "global_atomic_swap_x2" in asm and "cmpswap" not in asm
