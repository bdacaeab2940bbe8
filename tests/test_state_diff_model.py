"""The numpy model of the state diff (tests/state_diff_common.py model_diff) against hand-written cases -- what guards the model the GPU tests compare the device
with -- and the agreement of include/ggrs_hip.h, the ctypes mirror and rust/bevy_ggrs_hip/src/ffi.rs on the two structs and the GGRS_DIFF_* constants."""
import ctypes as C
import os
import re

import numpy as np

import state_diff_common as sd
from bevy_ggrs_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, U64 = np.uint32, np.uint64
COMPS = [(0, 0, 2), (2, 3, 1)]           # component 0: columns 0 and 1; component 1 (not rollback) owns column 2 and is not listed; component 2: column 3
NO = sd.NO_WORD


def side(n, alive, p0, p2, x, y, z, res=(1, 2)):
    b = lambda v: np.array(v, dtype=bool)
    return {"len": n, "alive": b(alive), "present": {0: b(p0), 2: b(p2)}, "words": {(0, 0): np.array(x, dtype=U32), (0, 1): np.array(y, dtype=U32), (2, 0): np.array(z, dtype=U64)},
            "res": {0: list(res)}}


def base(n=4):
    return side(n, [1] * n, [1] * n, [1] * n, list(range(n)), [7] * n, [9] * n)


def test_equal_states_do_not_differ():
    d = sd.model_diff(base(), base(), COMPS)
    assert d["n_entities"] == 0 and d["n_alive"] == 0 and d["entries"] == [] and d["n_presence"] == {} and d["n_value"] == {} and d["resource_diff"] == []


def test_dead_on_both_sides_with_different_bytes_is_no_difference():
    a, b = base(), base()
    for s in (a, b): s["alive"][2] = False
    a["words"][(0, 0)][2] = 1000; b["words"][(2, 0)][2] = 77; b["present"][0][2] = False
    assert sd.model_diff(a, b, COMPS)["n_entities"] == 0


def test_absent_on_both_sides_is_no_difference():
    a, b = base(), base()
    for s in (a, b): s["present"][2][1] = False
    a["words"][(2, 0)][1] = 1; b["words"][(2, 0)][1] = 2
    assert sd.model_diff(a, b, COMPS)["n_entities"] == 0


def test_words_are_compared_as_bits():
    a, b = base(), base()
    a["words"][(0, 1)] = np.array([0.0, -0.0, np.nan, 1.0], dtype=np.float32).view(U32)
    b["words"][(0, 1)] = np.array([-0.0, -0.0, np.nan, 1.0], dtype=np.float32).view(U32)
    b["words"][(0, 1)][2] ^= 1                                                 # another NaN payload
    d = sd.model_diff(a, b, COMPS)
    assert d["n_entities"] == 2 and d["n_value"] == {0: 2}
    assert d["entries"][0] == (0, 1, 1, 0, 1 << 1, 0, 1, 0x00000000, 0x80000000)
    assert d["entries"][1][0] == 2 and d["entries"][1][4] == 1 << 1 and d["entries"][1][7] ^ d["entries"][1][8] == 1


def test_len_on_one_side_only():
    a, b = base(4), base(6)
    d = sd.model_diff(a, b, COMPS)
    # slots 4 and 5 exist on side B alone: dead on A, alive on B -- only the alive bits are reported
    assert (d["len_a"], d["len_b"], d["n_entities"], d["n_alive"]) == (4, 6, 2, 2) and d["n_presence"] == {} and d["n_value"] == {}
    assert d["entries"] == [(4, 0, 1, 0, 0, NO, NO, 0, 0), (5, 0, 1, 0, 0, NO, NO, 0, 0)]
    b["alive"][5] = False                                                      # beyond A's len and dead on B: dead on both sides
    assert sd.model_diff(a, b, COMPS)["n_entities"] == 1


def test_alive_difference_hides_presence_and_values():
    a, b = base(), base()
    b["alive"][1] = False; b["present"][0][1] = False; b["words"][(2, 0)][1] = 5
    d = sd.model_diff(a, b, COMPS)
    assert d["entries"] == [(1, 1, 0, 0, 0, NO, NO, 0, 0)] and d["n_alive"] == 1 and d["n_presence"] == {} and d["n_value"] == {}


def test_presence_and_value_bits_and_the_lowest_column():
    a, b = base(), base()
    b["present"][2][0] = False                                                 # slot 0: component 2 on one side only
    b["words"][(0, 1)][3] = 8; b["words"][(2, 0)][3] = 1 << 40                 # slot 3: columns 1 and 3 differ, column 1 is the lowest
    b["words"][(2, 0)][0] = 55                                                 # slot 0's word of the one-sided component: not a value difference
    d = sd.model_diff(a, b, COMPS)
    assert d["n_entities"] == 2 and d["n_presence"] == {2: 1} and d["n_value"] == {0: 1, 2: 1}
    assert d["entries"] == [(0, 1, 1, 1 << 2, 0, NO, NO, 0, 0), (3, 1, 1, 0, (1 << 1) | (1 << 3), 0, 1, 7, 8)]


def test_truncation_and_ordering():
    n = 200
    a, b = base(n), base(n)
    hit = [199, 3, 64, 63, 128, 65]
    for s in hit: b["words"][(0, 0)][s] += 1
    for cap, want in ((0, []), (1, [3]), (4, [3, 63, 64, 65]), (6, sorted(hit)), (50, sorted(hit))):
        d = sd.model_diff(a, b, COMPS, max_entries=cap)
        assert [e[0] for e in d["entries"]] == want and d["n_entities"] == 6 and d["n_value"] == {0: 6}      # the counts are exact whatever the cap


def test_resources_word_by_word():
    a, b = base(), base()
    b["res"][0] = [1, 3]
    assert sd.model_diff(a, b, COMPS)["resource_diff"] == [0] and sd.model_diff(a, b, COMPS)["n_entities"] == 0


# ---- header, ctypes and ffi.rs agree
_C_SIZES = {"uint64_t": 8, "uint32_t": 4, "int32_t": 4}
_RS_SIZES = {"u64": 8, "u32": 4, "i32": 4}


def _layout(fields):
    """sizeof of a C struct of (size, count) fields under natural alignment."""
    off, al = 0, 1
    for size, count in fields:
        off = (off + size - 1) // size * size + size * count; al = max(al, size)
    return (off + al - 1) // al * al


def _header_struct(name):
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggrs_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s\s*;" % name, h).group(1)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(\w+)\s+(\w+)\s*(?:\[(\d+)\])?$", decl)
        out.append((m.group(2), _C_SIZES[m.group(1)], int(m.group(3) or 1)))
    return out


def _rust_struct(name):
    rs = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "ffi.rs")).read())
    body = re.search(r"pub struct %s\s*\{(.*?)\}" % name, rs, flags=re.S).group(1)
    out = []
    for m in re.finditer(r"pub (\w+):\s*(?:\[(\w+);\s*(\d+)\]|(\w+))", body):
        out.append((m.group(1), _RS_SIZES[m.group(2) or m.group(4)], int(m.group(3) or 1)))
    return out


def test_header_ctypes_and_rust_agree_on_the_structs_and_constants():
    for name, ct, size in (("ggrs_diff_entry", _ffi.DiffEntry, 56), ("ggrs_diff_report", _ffi.DiffReport, 1072)):
        hf, rf = _header_struct(name), _rust_struct(name)
        assert hf == rf, (name, hf, rf)
        assert [f[0] for f in ct._fields_] == [f[0] for f in hf], name
        for (fname, ftype), (_, fsize, count) in zip(ct._fields_, hf): assert C.sizeof(ftype) == fsize * count, (name, fname)
        assert C.sizeof(ct) == _layout([(s, c) for _, s, c in hf]) == size, name
    hdr = open(os.path.join(ROOT, "include", "ggrs_hip.h")).read()
    rs = open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "ffi.rs")).read()
    assert re.search(r"#define GGRS_DIFF_LIVE\s+INT32_MIN\b", hdr) and re.search(r"#define GGRS_DIFF_TRUST_VERSIONS\s+1u\b", hdr)
    assert _ffi.DIFF_LIVE == -(1 << 31) and _ffi.DIFF_TRUST_VERSIONS == 1
    assert int(re.search(r"pub const GGRS_DIFF_LIVE: i32 = (-?\d+);", rs).group(1)) == -(1 << 31)
    assert int(re.search(r"pub const GGRS_DIFF_TRUST_VERSIONS: u32 = (\d+);", rs).group(1)) == 1
    assert re.search(r"#define GGRS_HIP_ABI_VERSION 9\b", hdr)                  # new functions only: the version stays
