"""The delta's semantics and host checks without a GPU: the numpy model (tests/delta_common.py) held to hand-written cases for every kind, to the state diff's
model over the query fuzz's shadow states, and shown to be told from three deliberately wrong models; every refusal of ggrs_hip_delta_frames /
ggrs_hip_delta_block that needs no device, on a layout-only world; the new structs in the header, the ctypes binding and ffi.rs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import delta_common as dc
import query_common as qc
import state_diff_common as sd
from bevy_ggrs_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, U64 = np.uint32, np.uint64
POS0, NEG0, NAN_A, NAN_B = 0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001      # 0.0, -0.0 and two quiet NaNs as f32 bits


# ---------------------------------------------------------------------------------------------------------------- hand-written cases
def _pair():
    """OLD (len 6) and NEW (len 8) over eight slots; component 0 is one f32 word, component 1 one u64 word.
        0  alive on both; c0 equal; c1 inserted in NEW
        1  alive on both; c0 0.0 -> -0.0; c1 removed in NEW
        2  alive on both; c0 one NaN payload -> another
        3  dead on both (despawned before OLD), present bits and differing stale bytes left behind
        4  alive on both; c0 equal; c1 absent on both with different bytes under it
        5  alive in OLD, despawned in NEW (its bytes stay, one has even moved)
        6  at OLD's len: OLD's alive bit there is set and means nothing; spawned in NEW with c0
        7  beyond OLD's len: spawned and despawned again before NEW"""
    b = lambda *x: np.array(x, dtype=bool)
    old = {"len": 6, "alive": b(1, 1, 1, 0, 1, 1, 1, 0), "present": {0: b(1, 1, 1, 1, 1, 1, 1, 0), 1: b(0, 1, 0, 0, 0, 0, 0, 0)},
           "columns": {(0, 0): np.array([10, POS0, NAN_A, 111, 5, 77, 999, 0], dtype=U32), (1, 0): np.array([1, 2, 3, 4, 50, 6, 7, 8], dtype=U64)}}
    new = {"len": 8, "alive": b(1, 1, 1, 0, 1, 0, 1, 0), "present": {0: b(1, 1, 1, 1, 1, 1, 1, 1), 1: b(1, 0, 0, 0, 0, 0, 0, 0)},
           "columns": {(0, 0): np.array([10, NEG0, NAN_B, 222, 5, 78, 66, 1], dtype=U32), (1, 0): np.array([9, 2, 3, 4, 51, 6, 7, 8], dtype=U64)}}
    return old, new


FETCH = [(0, 0)]
# (kind, changed, forward: NEW against OLD, backward: OLD against NEW) -> the matching slots
HAND = [("changed", {0}, [1, 2, 6], [1, 2, 5]), ("changed", {1}, [0], [1]), ("changed", {0, 1}, [0, 1, 2, 6], [1, 2, 5]),
        ("added", {0}, [6], [5]), ("added", {1}, [0], [1]), ("added", {0, 1}, [0, 6], [1, 5]),
        ("removed", {0}, [5], [6]), ("removed", {1}, [1], [0]), ("removed", {0, 1}, [1, 5], [0, 6]),
        ("despawned", set(), [5], [6])]


def _slots(rec_new, rec_old, kind, changed, model=dc.model_delta, **kw):
    return model(rec_new, rec_old, dc.make_delta(kind, changed, **kw), 100)["all_slots"].tolist()


@pytest.mark.parametrize("kind,changed,fwd,bwd", HAND, ids=[f"{k}-{''.join(map(str, sorted(c)))}" for k, c, _, _ in HAND])
def test_hand_written_cases(kind, changed, fwd, bwd):
    old, new = _pair()
    assert _slots(new, old, kind, changed) == fwd                                                  # spawn, despawn, insert, remove, -0.0, NaN payloads, len_new > len_old
    assert _slots(old, new, kind, changed) == bwd                                                  # len_new < len_old


def test_hand_written_rows_words_and_report():
    old, new = _pair()
    r = dc.model_delta(new, old, dc.make_delta("changed", {0}, FETCH), 100)
    assert r["slots"].tolist() == [1, 2, 6] and r["columns"][0].tolist() == [NEG0, NAN_B, 66] and r["columns"][0].dtype == U32      # NEW's words
    assert (r["len_new"], r["len_old"], r["n_matched"], r["n_rows"], r["n_beyond_old_len"]) == (8, 6, 3, 3, 1)                      # slot 6 must be spawned first
    r = dc.model_delta(new, old, dc.make_delta("removed", {0}, FETCH), 100)
    assert r["slots"].tolist() == [5] and r["columns"][0].tolist() == [77] and r["n_beyond_old_len"] == 0                           # OLD's words: the last values
    r = dc.model_delta(new, old, dc.make_delta("despawned", (), [(0, 0), (1, 0)], slots=False), 100)
    assert r["n_matched"] == 0 and r["slots"] is None                                              # the fetched c1 is an implied With on OLD: slot 5 lacks it
    r = dc.model_delta(old, new, dc.make_delta("changed", {0}, FETCH), 100)
    assert r["columns"][0].tolist() == [POS0, NAN_A, 77] and (r["len_new"], r["len_old"], r["n_beyond_old_len"]) == (6, 8, 0)
    # max_rows cuts the rows, never the counts
    for cap, rows in ((0, []), (1, [1]), (2, [1, 2]), (3, [1, 2, 6]), (9, [1, 2, 6])):
        r = dc.model_delta(new, old, dc.make_delta("changed", {0}, FETCH), cap)
        assert r["slots"].tolist() == rows and (r["n_matched"], r["n_rows"], r["n_beyond_old_len"]) == (3, len(rows), 1)


def test_hand_written_filters_are_judged_on_the_base_side():
    old, new = _pair()
    assert _slots(new, old, "changed", {0}, with_=[1]) == []                                       # only slot 0 has c1 in NEW, and its c0 did not move
    assert _slots(new, old, "changed", {0, 1}, with_=[1]) == [0]
    assert _slots(new, old, "changed", {0}, without=[1]) == [1, 2, 6]                              # slot 1 lost c1: Without holds on NEW
    assert _slots(old, new, "changed", {0}, without=[1]) == [2, 5]                                 # ... and not on OLD
    assert _slots(new, old, "removed", {1}, with_=[0]) == [1] and _slots(new, old, "removed", {1}, without=[0]) == []
    assert _slots(new, old, "changed", {0, 1}) == [0, 1, 2, 6]                                     # a component of changed_mask is not an implied With: slot 6 has no c1
    assert _slots(new, old, "despawned", (), with_=[1]) == []


def test_masks_as_the_words_the_abi_hands_out():
    old, new = _pair()
    as_words = lambda m: np.array([int(sum(1 << i for i in range(m.size) if m[i]))], dtype=U64)
    for rec in (old, new): rec["alive"] = as_words(rec["alive"]); rec["present"] = {c: as_words(p) for c, p in rec["present"].items()}
    for kind, changed, fwd, bwd in HAND:
        assert _slots(new, old, kind, changed) == fwd and _slots(old, new, kind, changed) == bwd


@pytest.mark.parametrize("bug", dc.WRONG)
def test_wrong_models_are_caught_by_the_hand_written_cases(bug):
    old, new = _pair()
    wrong = dc.wrong_model(bug)
    caught = [(kind, sorted(changed), way) for kind, changed, fwd, bwd in HAND for way, (a, b, want) in (("forward", (new, old, fwd)), ("backward", (old, new, bwd)))
              if _slots(a, b, kind, changed, model=wrong) != want]
    assert caught, bug


# ---------------------------------------------------------------------------------------------------------------- against the state diff's model
def _diff_form(rec): return {"len": rec["len"], "alive": rec["alive"], "present": rec["present"], "words": rec["columns"]}


@pytest.mark.parametrize("seed", range(qc.FUZZ_SEEDS))
def test_union_of_the_kinds_is_what_the_state_diff_reports(seed):
    comps, rec0, live, _ = qc.fuzz_shadow_states(seed)
    every = set(range(len(comps)))
    col0, diff_comps = 0, []
    for c, (_, _, nw) in enumerate(comps): diff_comps.append((c, col0, nw)); col0 += nw
    for new, old in ((live, rec0), (rec0, live)):
        d = sd.model_diff(_diff_form(new), _diff_form(old), diff_comps, max_entries=1 << 30)
        differing = {e[0] for e in d["entries"]}
        changed = set(_slots(new, old, "changed", every))
        removed = set().union(*(set(_slots(new, old, "removed", {c})) for c in every))
        despawned = set(_slots(new, old, "despawned", ()))
        assert removed == set(_slots(new, old, "removed", every))
        # an entity alive in new only that holds no component there differs for the state diff (its alive bit) and is no Changed<C> row for any C
        bare = {s for s in differing if s < new["len"] and qc.as_bits(new["alive"], new["len"])[s] and not any(qc.as_bits(new["present"][c], new["len"])[s] for c in every)
                and not (s < old["len"] and qc.as_bits(old["alive"], old["len"])[s])}
        assert changed | removed | despawned == differing - bare, (seed, sorted((changed | removed | despawned) ^ differing))
        assert not (despawned - removed - {s for s in despawned if not any(qc.as_bits(old["present"][c], old["len"])[s] for c in every)})      # a despawn removes too


def test_wrong_models_are_caught_by_the_shadow_states():
    caught = {bug: 0 for bug in dc.WRONG}
    for seed in range(qc.FUZZ_SEEDS):
        comps, rec0, live, _ = qc.fuzz_shadow_states(seed)
        every = set(range(len(comps)))
        for new, old in ((live, rec0), (rec0, live)):
            for kind in dc.KINDS:
                changed = () if kind == "despawned" else every
                want = _slots(new, old, kind, changed)
                for bug in dc.WRONG: caught[bug] += _slots(new, old, kind, changed, model=dc.wrong_model(bug)) != want
    assert all(caught.values()), caught


# ---------------------------------------------------------------------------------------------------------------- refusals that need no device
STORE = ("__device__ void ggrs_store(const GgrsWords& t, GgrsWords& s) { s.u16(0) = (unsigned short)t.u32(0); }\n"
         "__device__ void ggrs_load(const GgrsWords& s, GgrsWords& t) { t.u32(0) = s.u16(0); }")


def _layout_world():
    w = bg.World(1000, max_depth=4, flags=bg.GGRS_WORLD_LAYOUT_ONLY)
    ids = {name: w.register_component(name, wb, nw) for name, wb, nw in qc.WIDTHS}
    ids["Side"] = w.register_component("Side", 4, 1, rollback=False)
    ids["Packed"] = w.register_component("Packed", 4, 1)
    w.register_component_strategy(ids["Packed"], 2, 1, STORE)
    return w, ids


def _call(w, desc, new=3, old=2, block=None, out=None, max_rows=0, report=True):
    rep = _ffi.DeltaReport()
    r = C.byref(rep) if report else None
    if block is None: rc = w._lib.ggrs_hip_delta_frames(w._p, new, old, C.byref(desc) if desc is not None else None, out, max_rows, r)
    else: rc = w._lib.ggrs_hip_delta_block(w._p, new, block, C.byref(desc) if desc is not None else None, out, max_rows, r)
    return rc, (w._lib.ggrs_hip_last_error(w._p) or b"").decode()


def _refused(w, desc, what, **kw):
    rc, msg = _call(w, desc, **kw)
    assert rc == bg.GGRS_E_INVALID and what in msg, (rc, msg, what)


def test_refusals_come_before_the_device_is_looked_at():
    w, i = _layout_world()
    D = w.delta_desc
    LIVE = bg.LIVE
    # everything the query refuses for q
    d = D([(i["B8"], 0)], changed=[i["B8"]]); d.q.words[0].comp = 17
    _refused(w, d, "component 17")
    _refused(w, D([(i["B8"], 2)], changed=[i["B8"]]), "word 2 of component B8")
    d = D(changed=[i["B8"]]); d.q.n_words = _ffi.QUERY_MAX_WORDS + 1
    _refused(w, d, "at most 32 words")
    _refused(w, D(changed=[i["B8"]], with_=[i["Mark"]], without=[i["Mark"]]), "With")
    _refused(w, D(changed=[i["B8"]], with_=[40]), "does not have")
    d = D(changed=[i["B8"]]); d.q.flags = 6
    _refused(w, d, "unknown query flags")
    # ... on the base side: NEW for changed / added, OLD for removed / despawned
    _refused(w, D(changed=[i["B8"]], with_=[i["Side"]]), "not registered for rollback")
    _refused(w, D([(i["Packed"], 0)], changed=[i["B8"]]), "under a Strategy")
    _refused(w, D(kind="removed", changed=[i["B8"]], without=[i["Side"]]), "not registered for rollback", new=LIVE, old=2)
    _refused(w, D([(i["Packed"], 0)], kind="despawned"), "under a Strategy", new=LIVE, block=C.c_void_p(4096))
    # the delta's own
    d = D(changed=[i["B8"]]); d.kind = 4
    _refused(w, d, "unknown delta kind 4")
    d = D(changed=[i["B8"]]); d.flags = 2
    _refused(w, d, "unknown delta flags 0x2")
    _refused(w, D(changed=[40]), "changed_mask 0x10000000000 names a component the world does not have")
    _refused(w, D(changed=[i["Side"]]), "Side, which is not registered for rollback")
    _refused(w, D(changed=[i["Side"]]), "Side, which is not registered for rollback", new=LIVE, old=2)
    _refused(w, D(kind="added", changed=[i["Side"]]), "Side, which is not registered for rollback", new=2, old=LIVE)
    for kind in ("changed", "added", "removed"): _refused(w, D(kind=kind), f"a delta {kind.upper()} with an empty changed_mask")
    _refused(w, D(kind="despawned", changed=[i["B8"]]), "in a delta DESPAWNED")
    _refused(w, D(changed=[i["Packed"]]), "live form and Stored form are not comparable", new=LIVE, old=2)
    _refused(w, D(changed=[i["Packed"]]), "live form and Stored form are not comparable", new=2, old=LIVE)
    _refused(w, D(changed=[i["Packed"]]), "live form and Stored form are not comparable", new=LIVE, block=C.c_void_p(4096))
    _refused(w, D(changed=[i["B8"]], trust_versions=True), "GGRS_DELTA_TRUST_VERSIONS with a foreign block", block=C.c_void_p(4096))
    _refused(w, D(changed=[i["B8"]]), "without a report", report=False)
    _refused(w, D(changed=[i["B8"]]), "max_rows 5 and no output buffer", max_rows=5)
    _refused(w, None, "without a desc")
    _refused(w, D(changed=[i["B8"]]), "without a block", block=C.c_void_p(0))
    assert w._lib.ggrs_hip_delta_frames(None, 1, 0, C.byref(D(changed=[i["B8"]])), None, 0, C.byref(_ffi.DeltaReport())) == bg.GGRS_E_INVALID
    with pytest.raises(ValueError): w.delta_desc(kind="moved")


def test_more_than_64_compared_columns_are_refused():
    w = bg.World(1000, max_depth=4, flags=bg.GGRS_WORLD_LAYOUT_ONLY)
    ids = [w.register_component(f"Wide{k}", 4, 13) for k in range(5)]                             # 65 columns
    _refused(w, w.delta_desc(changed=ids), "compares at most 64 columns, not 65")
    rc, _ = _call(w, w.delta_desc(changed=ids[:4]))
    assert rc == bg.GGRS_E_NO_DEVICE                                                               # 52 columns are served
    rc, _ = _call(w, w.delta_desc(kind="added", changed=ids))
    assert rc == bg.GGRS_E_NO_DEVICE                                                               # ADDED needs masks only


def test_a_good_descriptor_on_a_layout_only_world_says_no_device():
    w, i = _layout_world()
    D = w.delta_desc
    good = [(D([(i["B8"], 0)], changed=[i["B16"], i["B64"]], without=[i["Mark"]]), {}), (D(kind="added", changed=[i["Packed"]]), {"new": bg.LIVE}),
            (D(kind="removed", changed=[i["Packed"]], with_=[i["Packed"]]), {}), (D([(i["B32"], 1)], kind="despawned"), {"old": bg.LIVE}),
            (D(changed=[i["Packed"]]), {}), (D(changed=[i["Packed"], i["Side"]], with_=[i["Side"]]), {"new": bg.LIVE, "old": bg.LIVE}),
            (D(changed=[i["B8"]], trust_versions=True), {}), (D([(i["Packed"], 0)], changed=[i["B8"]]), {"new": bg.LIVE}),
            (D(changed=[i["B8"]]), {"block": C.c_void_p(4096)})]
    for desc, kw in good:
        rc, msg = _call(w, desc, **kw)
        assert rc == bg.GGRS_E_NO_DEVICE and msg, (rc, msg, kw)


# ---------------------------------------------------------------------------------------------------------------- header <-> ctypes <-> ffi.rs
def test_delta_structs_agree_between_header_ctypes_and_ffi_rs():
    from test_abi import _parse_ffi_rs, _parse_header
    c_fns, c_structs = _parse_header()
    r_fns, r_structs = _parse_ffi_rs()
    hdr = open(os.path.join(ROOT, "include", "ggrs_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (GGRS_DELTA_[A-Z_]+)\s+(\d+)u?", hdr)}
    assert consts == {"GGRS_DELTA_CHANGED": 0, "GGRS_DELTA_ADDED": 1, "GGRS_DELTA_REMOVED": 2, "GGRS_DELTA_DESPAWNED": 3, "GGRS_DELTA_TRUST_VERSIONS": 1}
    assert _ffi.DELTA_KINDS == {"changed": 0, "added": 1, "removed": 2, "despawned": 3} and _ffi.DELTA_TRUST_VERSIONS == 1
    rs = open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "ffi.rs")).read()
    for name, v in consts.items(): assert re.search(r"pub const %s: u32 = %d;" % (name, v), rs), name
    ct = {"ggrs_delta_desc": _ffi.DeltaDesc, "ggrs_delta_report": _ffi.DeltaReport}
    sizes = {"ggrs_delta_desc": 24 + 32 * 8 + 16, "ggrs_delta_report": 40}
    for name, cls in ct.items():
        assert name in c_structs and name in r_structs, name
        assert r_structs[name] == c_structs[name], f"{name}: ffi.rs {r_structs[name]} vs header {c_structs[name]}"
        assert [f[0] for f in cls._fields_] == [n for n, _ in c_structs[name]], name
        assert C.sizeof(cls) == sizes[name], (name, C.sizeof(cls))
    for fn in ("ggrs_hip_delta_frames", "ggrs_hip_delta_block"):
        assert r_fns[fn] == c_fns[fn] and len(_ffi.SIGNATURES[fn][1]) == len(c_fns[fn][1]), fn
    assert [n for n, _ in c_fns["ggrs_hip_delta_frames"][1]] == ["w", "frame_new", "frame_old", "desc", "out_dev", "max_rows", "report"]
    assert [n for n, _ in c_fns["ggrs_hip_delta_block"][1]] == ["w", "frame_new", "block_old_dev", "desc", "out_dev", "max_rows", "report"]
    assert _ffi.lib.ggrs_hip_abi_version() == 9 and bg.DeltaResult is not None and issubclass(bg.DeltaResult, bg.QueryResult) and hasattr(bg.World, "delta")
    lib_rs = open(os.path.join(ROOT, "rust", "bevy_ggrs_hip", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "bevy_ggrs_hip.hpp")).read()
    assert "pub unsafe fn delta(" in lib_rs and all(f" {m}(" in hpp for m in ("delta_desc", "delta_frames", "delta_block"))
