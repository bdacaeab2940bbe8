"""The scatter without a device: the numpy model of its semantics (tests/scatter_common.py) against hand-written cases and against the CPU oracle driven one slot
at a time (apply_per_slot), and what ggrs_hip_scatter refuses before it looks at the device -- every descriptor refusal, with its message, on a
GGRS_WORLD_LAYOUT_ONLY world, and GGRS_E_NO_DEVICE for a good descriptor there."""
import ctypes as C

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import query_common as qc
import scatter_common as sc
from bevy_ggrs_amd import _ffi
from oracle.binding import OracleWorld

U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64


# ---------------------------------------------------------------------------------------------------------------- the model against hand-written cases
def tiny():
    """Six slots, len 5 (slot 5 is beyond it); slot 1 is dead; component 0 {2 x u32} is missing on slot 3, component 1 {1 x u8} is only on slots 0 and 4."""
    return {"len": 5, "alive": np.array([1, 0, 1, 1, 1, 0], dtype=bool),
            "present": {0: np.array([1, 1, 1, 0, 1, 0], dtype=bool), 1: np.array([1, 0, 0, 0, 1, 0], dtype=bool)},
            "columns": {(0, 0): np.arange(10, 16, dtype=U32), (0, 1): np.arange(20, 26, dtype=U32), (1, 0): np.arange(30, 36, dtype=U8)}}


def test_write_applies_where_alive_and_present():
    rec = tiny()
    out, rep = sc.model_scatter(rec, sc.make_sdesc("write", [(0, 1)]), [0, 1, 2, 3, 4], [np.array([100, 101, 102, 103, 104], dtype=U32)])
    assert rep == {"len": 5, "n_rows": 5, "n_applied": 3, "n_dead": 1, "n_absent": 1, "first_bad_row": None}                # slot 1 is dead, slot 3 lacks component 0
    assert out["columns"][(0, 1)].tolist() == [100, 21, 102, 23, 104, 25] and out["columns"][(0, 0)].tolist() == rec["columns"][(0, 0)].tolist()
    assert out["alive"].tolist() == rec["alive"].tolist() and all(out["present"][c].tolist() == rec["present"][c].tolist() for c in (0, 1))
    # words of two components: every named component must be present (slot 2 lacks component 1)
    out, rep = sc.model_scatter(rec, sc.make_sdesc("write", [(1, 0), (0, 0)]), [0, 2, 4], [np.array([1, 2, 3], dtype=U8), np.array([7, 8, 9], dtype=U32)])
    assert (rep["n_applied"], rep["n_dead"], rep["n_absent"]) == (2, 0, 1)
    assert out["columns"][(1, 0)].tolist() == [1, 31, 32, 33, 3, 35] and out["columns"][(0, 0)].tolist() == [7, 11, 12, 13, 9, 15]
    assert rec["columns"][(0, 0)].tolist() == list(range(10, 16))                                                           # the input record is left alone


def test_insert_sets_presence_and_replaces_words_on_alive_slots_only():
    rec = tiny()
    out, rep = sc.model_scatter(rec, sc.make_sdesc("insert", [(0, 1), (0, 0)]), [1, 3, 4], [np.array([5, 6, 7], dtype=U32), np.array([50, 60, 70], dtype=U32)])
    assert (rep["n_applied"], rep["n_dead"], rep["n_absent"]) == (2, 1, 0)                                                  # an insert knows no absence; slot 1 is dead
    assert out["present"][0].tolist() == [1, 1, 1, 1, 1, 0] and out["present"][1].tolist() == rec["present"][1].tolist()
    assert out["columns"][(0, 0)].tolist() == [10, 11, 12, 60, 70, 15] and out["columns"][(0, 1)].tolist() == [20, 21, 22, 6, 7, 25]   # slot 4 had it: replaced


def test_remove_and_despawn():
    rec = tiny()
    out, rep = sc.model_scatter(rec, sc.make_sdesc("remove", comps=[0, 1]), [0, 1, 3])
    assert (rep["n_applied"], rep["n_dead"], rep["n_absent"]) == (2, 1, 0)                                                  # slot 3 lacks component 0: still applied
    assert out["present"][0].tolist() == [0, 1, 1, 0, 1, 0] and out["present"][1].tolist() == [0, 0, 0, 0, 1, 0] and out["alive"].tolist() == rec["alive"].tolist()
    assert all(out["columns"][k].tolist() == rec["columns"][k].tolist() for k in rec["columns"])
    out, rep = sc.model_scatter(rec, sc.make_sdesc("despawn"), [1, 2, 4])
    assert (rep["n_applied"], rep["n_dead"], rep["n_absent"]) == (2, 1, 0)
    assert out["alive"].tolist() == [1, 0, 0, 1, 0, 0] and all(out["present"][c].tolist() == rec["present"][c].tolist() for c in (0, 1))


@pytest.mark.parametrize("slots, bad", [([0, 5], 1), ([5], 0), ([2, 2, 3], 1), ([0, 3, 3], 2), ([3, 2], 1), ([0, 4, 1, 0], 2), ([0, 1, 2, 3, 4, 5], 5), ([4, 0, 9], 1)])
def test_bad_rows_change_nothing_and_name_the_lowest(slots, bad):
    rec = tiny()
    for desc, cols in ((sc.make_sdesc("write", [(0, 0)]), [np.full(len(slots), 99, dtype=U32)]), (sc.make_sdesc("despawn"), []), (sc.make_sdesc("remove", comps=[0]), []),
                       (sc.make_sdesc("insert", [(1, 0)]), [np.full(len(slots), 9, dtype=U8)])):
        out, rep = sc.model_scatter(rec, desc, slots, cols)
        assert rep == {"len": 5, "n_rows": len(slots), "n_applied": 0, "n_dead": 0, "n_absent": 0, "first_bad_row": bad}
        sc.assert_records_equal(out, rec, (slots, desc["op"]))


def test_no_rows_is_a_no_op_with_a_report():
    rec = tiny()
    for desc, cols in ((sc.make_sdesc("write", [(0, 0)]), [np.zeros(0, dtype=U32)]), (sc.make_sdesc("despawn"), [])):
        out, rep = sc.model_scatter(rec, desc, [], cols)
        assert rep == {"len": 5, "n_rows": 0, "n_applied": 0, "n_dead": 0, "n_absent": 0, "first_bad_row": None}
        sc.assert_records_equal(out, rec)


def test_masks_as_download_words():
    rec = tiny()
    rec["alive"] = np.array([0b011101], dtype=U64); rec["present"][0] = np.array([0b010111], dtype=U64)
    out, rep = sc.model_scatter(rec, sc.make_sdesc("write", [(0, 0)]), [1, 3, 4], [np.array([1, 2, 3], dtype=U32)])
    assert (rep["n_applied"], rep["n_dead"], rep["n_absent"]) == (1, 1, 1) and out["columns"][(0, 0)].tolist() == [10, 11, 12, 13, 3, 15]


# ---------------------------------------------------------------------------------------------------------------- the model against the oracle, slot by slot
N = 300


def widths_world():
    w = OracleWorld(N + 40, 4)
    ids = qc.build_widths(w)
    qc.spawn_widths(w, ids, N)
    for s in range(0, N, 7): w.insert_component(ids["Mark"], s, np.array([s ^ 0x5A5A5A], dtype=U32))
    for s in range(0, N, 11): w.remove_component(ids["B16"], s)
    for s in sorted(set(range(0, N, 13)) | set(range(64, 128))): w.despawn(s)
    return w, ids


def rows_and_values(w, words, seed):
    r = np.random.default_rng([77, seed])
    slots = np.flatnonzero(r.random(N) < 0.4)                                                      # ascending, dead slots and slots without the component left in
    cols = [r.integers(0, 2 ** (8 * w._comps[c][1]), slots.size, dtype=U64).astype(qc.UINT[w._comps[c][1]]) for c, _ in words]
    return slots, cols


@pytest.mark.parametrize("op", sc.OPS)
def test_model_equals_the_oracle_driven_per_slot(op):
    w, ids = widths_world()
    every = qc.all_words(w, ids, ("B64", "B8", "B16", "B32", "Mark"))
    words = {"write": [every[k] for k in (1, 3, 0, 6, 8, 5)], "insert": qc.all_words(w, ids, ("Mark", "B16")), "remove": [], "despawn": []}[op]
    desc = sc.make_sdesc(op, words, comps=[ids["B16"], ids["Mark"]] if op == "remove" else ())
    before = sc.full_record(w)
    slots, cols = rows_and_values(w, words, sc.OPS.index(op))
    want, rep = sc.model_scatter(before, desc, slots, cols)
    got_rep = sc.apply_per_slot(w, desc, slots, cols)
    assert got_rep == rep and rep["first_bad_row"] is None
    assert rep["n_applied"] and rep["n_dead"] and (rep["n_absent"] or op != "write") and rep["n_applied"] + rep["n_dead"] + rep["n_absent"] == slots.size
    sc.assert_records_equal(sc.full_record(w), want, op)
    # refused rows leave the oracle alone, too
    bad = np.concatenate([slots[:5], slots[4:9]])
    want2, rep2 = sc.model_scatter(want, desc, bad, [np.concatenate([c[:5], c[4:9]]) for c in cols])
    assert rep2["first_bad_row"] == 5 and sc.apply_per_slot(w, desc, bad, [np.concatenate([c[:5], c[4:9]]) for c in cols]) == rep2
    sc.assert_records_equal(sc.full_record(w), want, op + ", refused")
    w.close()


# ---------------------------------------------------------------------------------------------------------------- what is refused before the device is looked at
@pytest.fixture(scope="module")
def layout_world():
    w = bg.World(1000, max_depth=4, flags=bg.GGRS_WORLD_LAYOUT_ONLY)
    ids = qc.build_widths(w)
    yield w, ids
    w.close()


def call(w, op, words=(), comp_mask=0, *, flags=0, n_words=None, in_dev=0x1000, stride=8, n_rows=8, report=True):
    d = _ffi.ScatterDesc()
    d.op, d.flags, d.comp_mask, d.n_words = op, flags, comp_mask, len(words) if n_words is None else n_words
    for k, (c, wd) in enumerate(words): d.words[k].comp = c; d.words[k].word = wd
    rep = _ffi.ScatterReport()
    rc = w._lib.ggrs_hip_scatter(w._p, C.byref(d), in_dev or None, stride, n_rows, C.byref(rep) if report else None)
    return rc, w._lib.ggrs_hip_last_error(w._p).decode()


def test_every_descriptor_refusal_has_its_message(layout_world):
    w, ids = layout_world
    W, I, R, D = _ffi.SCATTER_WRITE, _ffi.SCATTER_INSERT, _ffi.SCATTER_REMOVE, _ffi.SCATTER_DESPAWN
    b32, b16, mark = ids["B32"], ids["B16"], ids["Mark"]
    cases = [
        (dict(op=4, words=[(b32, 0)]), "unknown scatter op 4"),
        (dict(op=W, words=[(b32, 0)], flags=1), "unknown scatter flags 0x1"),
        (dict(op=W, words=[(9, 0)]), "names component 9: the world has 5"),
        (dict(op=W, words=[(b32, 2)]), "names word 2 of component B32, which has 2"),
        (dict(op=W, words=[(b32, 0), (b16, 1), (b32, 0)]), "scatter words 0 and 2 both name word 0 of component B32"),
        (dict(op=W), "a scatter WRITE names no word"),
        (dict(op=I), "a scatter INSERT names no word"),
        (dict(op=W, words=[(b32, 0)], n_words=33), "at most 32 words, not 33"),
        (dict(op=R, words=[(b32, 0)], comp_mask=1 << b32), "a scatter REMOVE carries no words, not 1"),
        (dict(op=D, words=[(b32, 0)]), "a scatter DESPAWN carries no words, not 1"),
        (dict(op=W, words=[(b32, 0)], comp_mask=1 << b32), "in a scatter WRITE: it names what REMOVE removes"),
        (dict(op=I, words=[(mark, 0)], comp_mask=1 << mark), "in a scatter INSERT: it names what REMOVE removes"),
        (dict(op=D, comp_mask=2), "in a scatter DESPAWN: it names what REMOVE removes"),
        (dict(op=R), "a scatter REMOVE with an empty comp_mask removes nothing"),
        (dict(op=R, comp_mask=1 << 5), "a scatter REMOVE names a component the world does not have"),
        (dict(op=I, words=[(b16, 0), (b16, 2)]), "a scatter INSERT names 2 of the 3 words of component B16"),
        (dict(op=W, words=[(b32, 0)], in_dev=0), "scatter of 8 rows and no input buffer"),
        (dict(op=D, in_dev=0), "scatter of 8 rows and no input buffer"),
        (dict(op=W, words=[(b32, 0)], stride=7), "scatter of 8 rows from a buffer laid out for 7"),
        (dict(op=W, words=[(b32, 0)], report=False), "scatter without a report"),
    ]
    for kw, msg in cases:
        rc, err = call(w, **kw)
        assert rc == bg.GGRS_E_INVALID and msg in err, (kw, rc, err)
    rep = _ffi.ScatterReport()
    assert w._lib.ggrs_hip_scatter(w._p, None, 0x1000, 8, 8, C.byref(rep)) == bg.GGRS_E_INVALID and "scatter without a desc" in w._lib.ggrs_hip_last_error(w._p).decode()


def test_a_good_descriptor_on_a_layout_only_world_is_no_device(layout_world):
    w, ids = layout_world
    W, I, R, D = _ffi.SCATTER_WRITE, _ffi.SCATTER_INSERT, _ffi.SCATTER_REMOVE, _ffi.SCATTER_DESPAWN
    good = [dict(op=W, words=[(ids["B32"], 1), (ids["B8"], 0), (ids["B64"], 1)]), dict(op=I, words=qc.all_words(w, ids, ("B16", "Mark"))),
            dict(op=R, comp_mask=(1 << ids["Mark"]) | (1 << ids["B8"])), dict(op=D), dict(op=D, in_dev=0, n_rows=0, stride=0), dict(op=W, words=[(ids["B8"], 1)], n_rows=0)]
    for kw in good:
        rc, err = call(w, **kw)
        assert rc == bg.GGRS_E_NO_DEVICE and "layout-only" in err, (kw, rc, err)


def test_python_surface_without_a_device(layout_world):
    w, ids = layout_world
    d = w.scatter_desc("remove", comps=[ids["Mark"], ids["B8"]])
    assert (d.op, d.comp_mask, d.n_words) == (_ffi.SCATTER_REMOVE, (1 << ids["Mark"]) | (1 << ids["B8"]), 0)
    d = w.scatter_desc("insert", [(ids["Mark"], 0)])
    assert (d.op, d.n_words, d.words[0].comp, d.words[0].word) == (_ffi.SCATTER_INSERT, 1, ids["Mark"], 0)
    with pytest.raises(ValueError): w.scatter_desc("upsert")
    assert C.sizeof(_ffi.ScatterDesc) == 24 + 8 * _ffi.QUERY_MAX_WORDS and C.sizeof(_ffi.ScatterReport) == 48
    r = bg.ScatterReport(len=5, n_rows=3, n_applied=1, n_dead=1, n_absent=1, first_bad_row=None)
    assert r.n_applied + r.n_dead + r.n_absent == r.n_rows
