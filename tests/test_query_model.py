"""The query's semantics and host arithmetic without a GPU: the numpy model (tests/query_common.py) held to hand-written cases, ggrs_hip_query_layout on a
layout-only world (alignment, order, the four word widths, slots on and off, total_bytes, every refusal that needs no device), and the new structs in the header,
the ctypes binding and ffi.rs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import query_common as qc
from bevy_ggrs_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64


# ---------------------------------------------------------------------------------------------------------------- the model
def _tiny():
    """Ten slots, len 8: slot 8 has its alive bit set beyond len.  Component 0 everywhere, component 1 on even slots, component 2 on slots 1, 2, 3."""
    alive = np.array([1, 1, 0, 1, 1, 1, 0, 1, 1, 0], dtype=bool)
    present = {0: np.ones(10, dtype=bool), 1: np.arange(10) % 2 == 0, 2: np.isin(np.arange(10), (1, 2, 3))}
    columns = {(0, 0): (np.arange(10) * 10).astype(U32), (0, 1): (np.arange(10) + 100).astype(U64), (1, 0): (np.arange(10) + 50).astype(U8), (2, 0): (np.arange(10) * 3).astype(U16)}
    return alive, 8, present, columns


def test_model_len_cuts_a_set_alive_bit():
    alive, n, present, columns = _tiny()
    r = qc.model_query(alive, n, present, columns, qc.make_desc([(0, 0)]), 100)
    assert r["slots"].tolist() == [0, 1, 3, 4, 5, 7] and r["n_matched"] == 6 and r["columns"][0].tolist() == [0, 10, 30, 40, 50, 70]
    r = qc.model_query(alive, 10, present, columns, qc.make_desc([(0, 0)]), 100)
    assert r["slots"].tolist() == [0, 1, 3, 4, 5, 7, 8]                                           # with len 10 the bit counts
    # the same masks as the uint64 words the C ABI hands out
    words = np.array([int(sum(1 << i for i in range(10) if alive[i]))], dtype=U64)
    r = qc.model_query(words, n, present, columns, qc.make_desc([(0, 0)]), 100)
    assert r["slots"].tolist() == [0, 1, 3, 4, 5, 7]


def test_model_filters():
    alive, n, present, columns = _tiny()
    q = lambda **kw: qc.model_query(alive, n, present, columns, qc.make_desc(**kw), 100)
    assert q(with_=[1])["slots"].tolist() == [0, 4]                                               # With
    assert q(without=[1])["slots"].tolist() == [1, 3, 5, 7]                                       # Without
    assert q(with_=[2], without=[1])["slots"].tolist() == [1, 3]                                  # both
    assert q(with_=[1, 2])["slots"].tolist() == [] and q(with_=[1, 2])["n_matched"] == 0          # empty (slot 2 has both and is dead)
    assert q()["slots"].tolist() == [0, 1, 3, 4, 5, 7] and q()["columns"] == []                   # no filter: every live entity below len
    assert q(slots=False)["slots"] is None and q(slots=False)["n_matched"] == 6


def test_model_fetched_component_is_an_implicit_with():
    alive, n, present, columns = _tiny()
    r = qc.model_query(alive, n, present, columns, qc.make_desc([(2, 0), (0, 1)]), 100)
    assert r["slots"].tolist() == [1, 3] and r["columns"][0].tolist() == [3, 9] and r["columns"][1].tolist() == [101, 103]
    assert r["columns"][0].dtype == U16 and r["columns"][1].dtype == U64
    r = qc.model_query(alive, n, present, columns, qc.make_desc([(1, 0)], without=[2]), 100)
    assert r["slots"].tolist() == [0, 4] and r["columns"][0].tolist() == [50, 54]


def test_model_max_rows():
    alive, n, present, columns = _tiny()
    for cap, rows in ((0, []), (3, [0, 1, 3]), (6, [0, 1, 3, 4, 5, 7]), (7, [0, 1, 3, 4, 5, 7])):
        r = qc.model_query(alive, n, present, columns, qc.make_desc([(0, 0)]), cap)
        assert r["n_matched"] == 6 and r["n_rows"] == len(rows) and r["slots"].tolist() == rows and r["columns"][0].tolist() == [10 * s for s in rows]


def test_expected_buffer_layout():
    alive, n, present, columns = _tiny()
    r = qc.model_query(alive, n, present, columns, qc.make_desc([(1, 0), (0, 1)]), 3)
    buf = qc.expected_buffer(r, [1, 8], 3, 1024)
    assert buf[:2].tolist() == [50, 54] and (buf[2:256] == qc.FILL).all()                          # two rows of a u8 column, the third row and the padding untouched
    assert buf[256:272].view(U64).tolist() == [100, 104] and (buf[272:512] == qc.FILL).all()
    assert buf[512:520].view(U32).tolist() == [0, 4] and (buf[520:] == qc.FILL).all()


# ---------------------------------------------------------------------------------------------------------------- ggrs_hip_query_layout
def _layout_world(capacity=1000):
    w = bg.World(capacity, max_depth=4, flags=bg.GGRS_WORLD_LAYOUT_ONLY)
    ids = {name: w.register_component(name, wb, nw) for name, wb, nw in qc.WIDTHS}
    return w, ids


def test_layout_alignment_order_widths_and_total():
    w, ids = _layout_world()
    fetch = [(ids["B64"], 1), (ids["B8"], 0), (ids["B32"], 1), (ids["B16"], 2), (ids["B8"], 1)]               # permuted, all four widths
    for max_rows in (0, 1, 63, 64, 255, 256, 257, 1000):
        for slots in (True, False):
            lay = w.query_layout(w.query_desc(fetch, slots=slots), max_rows)
            offs, s_off, total = qc.model_layout([8, 1, 4, 2, 1], slots, max_rows)
            assert [int(lay.col_off[k]) for k in range(5)] == offs and [int(lay.word_bytes[k]) for k in range(5)] == [8, 1, 4, 2, 1]
            assert all(o % 256 == 0 for o in offs) and offs == sorted(offs)
            assert int(lay.total_bytes) == total and total % 256 == 0
            if slots: assert int(lay.slots_off) == s_off and s_off % 256 == 0 and s_off >= offs[-1] + max_rows and total >= s_off + 4 * max_rows
            for k in range(4): assert offs[k + 1] >= offs[k] + max_rows * [8, 1, 4, 2, 1][k]                 # columns do not overlap
    # a component id stands for all of its words, in order
    d = w.query_desc([ids["B16"], (ids["B64"], 0)])
    assert d.n_words == 4 and [(d.words[k].comp, d.words[k].word) for k in range(4)] == [(ids["B16"], 0), (ids["B16"], 1), (ids["B16"], 2), (ids["B64"], 0)]
    # slots only
    lay = w.query_layout(w.query_desc([], slots=True), 100)
    assert int(lay.slots_off) == 0 and int(lay.total_bytes) == 512
    assert int(w.query_layout(w.query_desc([], slots=False), 100).total_bytes) == 0


def _refused(w, desc, what):
    lay = _ffi.QueryLayout()
    rc = w._lib.ggrs_hip_query_layout(w._p, C.byref(desc), 10, C.byref(lay))
    msg = w._lib.ggrs_hip_last_error(w._p).decode()
    assert rc == bg.GGRS_E_INVALID and what in msg, (rc, msg)


def test_layout_refusals_that_need_no_device():
    w, ids = _layout_world()
    d = w.query_desc([(ids["B8"], 0)]); d.words[0].comp = 17
    _refused(w, d, "component 17")                                                                 # a component the world does not have
    _refused(w, w.query_desc([(ids["B8"], 2)]), "word 2 of component B8")                            # a word beyond the component
    d = w.query_desc([]); d.n_words = _ffi.QUERY_MAX_WORDS + 1
    _refused(w, d, "at most 32 words")
    _refused(w, w.query_desc([], with_=[ids["Mark"]], without=[ids["Mark"]]), "With")               # the same bit in both masks
    _refused(w, w.query_desc([(ids["B32"], 0)], without=[ids["B32"]]), "With")                      # ... also where the With is a fetch's
    _refused(w, w.query_desc([], with_=[9]), "does not have")                                       # a filter bit beyond the components
    _refused(w, w.query_desc([], without=[63]), "does not have")
    d = w.query_desc([]); d.flags = 6
    _refused(w, d, "unknown query flags")
    assert w._lib.ggrs_hip_query_layout(w._p, None, 10, C.byref(_ffi.QueryLayout())) == bg.GGRS_E_INVALID
    assert w._lib.ggrs_hip_query_layout(w._p, C.byref(w.query_desc([])), 10, None) == bg.GGRS_E_INVALID
    # exactly GGRS_QUERY_MAX_WORDS words are served
    lay = w.query_layout(w.query_desc([(ids["B64"], 0)] * _ffi.QUERY_MAX_WORDS, slots=False), 3)
    assert int(lay.col_off[31]) == 31 * 256 and int(lay.total_bytes) == 32 * 256
    # slots are 32-bit.  query_check refuses GGRS_QUERY_SLOTS in a world of more than 2^32 slots, but no such world exists today: world creation stops at 2^28
    # (32-bit lane offsets in the kernels), so that refusal cannot be reached through the ABI and the largest world there is gets its slots
    with pytest.raises(bg.GgrsHipError) as e: _layout_world((1 << 32) + 1)
    assert e.value.code == bg.GGRS_E_INVALID
    top, tids = _layout_world(1 << 28)
    assert int(top.query_layout(top.query_desc([], slots=True), 10).total_bytes) == 256


def test_query_calls_on_a_layout_only_world_say_no_device():
    w, ids = _layout_world()
    d, rep = w.query_desc([(ids["B8"], 0)]), _ffi.QueryReport()
    assert w._lib.ggrs_hip_query(w._p, bg.LIVE, C.byref(d), None, 0, C.byref(rep)) == bg.GGRS_E_NO_DEVICE and w._lib.ggrs_hip_last_error(w._p)
    assert w._lib.ggrs_hip_query_block(w._p, C.c_void_p(4096), C.byref(d), None, 0, C.byref(rep)) == bg.GGRS_E_NO_DEVICE and w._lib.ggrs_hip_last_error(w._p)


# ---------------------------------------------------------------------------------------------------------------- header <-> ctypes <-> ffi.rs
def test_query_structs_agree_between_header_ctypes_and_ffi_rs():
    from test_abi import _parse_ffi_rs, _parse_header
    c_fns, c_structs = _parse_header()
    r_fns, r_structs = _parse_ffi_rs()
    hdr = open(os.path.join(ROOT, "include", "ggrs_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (GGRS_QUERY_[A-Z_]+)\s+(\d+)u?", hdr)}
    assert consts == {"GGRS_QUERY_MAX_WORDS": 32, "GGRS_QUERY_SLOTS": 1} and _ffi.QUERY_MAX_WORDS == 32 and _ffi.QUERY_SLOTS == 1
    rs = open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "ffi.rs")).read()
    assert re.search(r"pub const GGRS_QUERY_MAX_WORDS: usize = 32;", rs) and re.search(r"pub const GGRS_QUERY_SLOTS: u32 = 1;", rs)
    ct = {"ggrs_query_word": _ffi.QueryWord, "ggrs_query_desc": _ffi.QueryDesc, "ggrs_query_layout": _ffi.QueryLayout, "ggrs_query_report": _ffi.QueryReport}
    sizes = {"ggrs_query_word": 8, "ggrs_query_desc": 24 + 32 * 8, "ggrs_query_layout": 16 + 32 * 8 + 32 * 4, "ggrs_query_report": 24}
    for name, cls in ct.items():
        assert name in c_structs and name in r_structs, name
        assert r_structs[name] == c_structs[name], f"{name}: ffi.rs {r_structs[name]} vs header {c_structs[name]}"
        assert [f[0] for f in cls._fields_] == [n for n, _ in c_structs[name]], name              # the same field names in the same order
        assert C.sizeof(cls) == sizes[name], (name, C.sizeof(cls))
    for fn in ("ggrs_hip_query_layout", "ggrs_hip_query", "ggrs_hip_query_block"):
        assert r_fns[fn] == c_fns[fn] and len(_ffi.SIGNATURES[fn][1]) == len(c_fns[fn][1]), fn
    assert [n for n, _ in c_fns["ggrs_hip_query"][1]] == ["w", "frame", "desc", "out_dev", "max_rows", "report"]


def test_abi_version_is_still_9():
    assert _ffi.lib.ggrs_hip_abi_version() == 9
    assert re.search(r"#define GGRS_HIP_ABI_VERSION\s+9\b", open(os.path.join(ROOT, "include", "ggrs_hip.h")).read())
    assert bg.QueryResult is not None and hasattr(bg.World, "query")
