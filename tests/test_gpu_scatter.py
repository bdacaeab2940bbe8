"""The device scatter (ggrs_hip_scatter; World.scatter) against the numpy model of its semantics (tests/scatter_common.py).  Every comparison is the WHOLE live
state -- every word of every component over [0, capacity), the alive mask, every presence mask -- after the call against the model over a record taken before it,
bit for bit: untouched slots and columns are checked too.  The bookkeeping cases hold a session on the device against the CPU oracle, which gets the same edit
one slot at a time (apply_per_slot), through Saves and rollback Loads."""
import ctypes as C

import numpy as np
import pytest
import torch

import bevy_ggrs_amd as bg
import common as cm
import query_common as qc
import scatter_common as sc
from bevy_ggrs_amd import _ffi
from oracle.binding import OracleWorld

pytestmark = pytest.mark.gpu

U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
S, L, A = bg.SaveGameState, bg.LoadGameState, bg.AdvanceFrame
GRIDS = (0, 1, 2, 7)                                                                               # by size, then capped to 1, 2 and 7 workgroups
TILE = 8192


# ---------------------------------------------------------------------------------------------------------------- the edge worlds
def build_edge(w, n):
    """n entities with every word width.  Mark sits on every 7th slot, B16 is removed from every 11th; every slot s with s % 13 == 5 is despawned and unit 1 (slots
    64..127) is wholly dead -- as far as n reaches.  Frame 0 is saved: a Load of it puts the world back."""
    ids = qc.build_widths(w)
    w.set_depth(4)
    qc.spawn_widths(w, ids, n)
    for s in range(0, n, 7): w.insert_component(ids["Mark"], s, np.array([s ^ 0x5A5A5A], dtype=U32))
    for s in range(0, n, 11): w.remove_component(ids["B16"], s)
    for s in sorted(x for x in set(range(5, n, 13)) | set(range(64, 128)) if x < n): w.despawn(s)
    w.handle_requests([S(0)])
    return ids


class Edge:
    def __init__(self, n):
        self.n = n
        self.w = bg.World(n + 200, max_depth=4)
        self.ids = build_edge(self.w, n)
        self.base = sc.full_record(self.w)
        assert self.base["len"] == n

    def descs(self):
        i = self.ids
        return {"write": sc.make_sdesc("write", [(i["B64"], 1), (i["B8"], 0), (i["B32"], 1), (i["B16"], 2), (i["B8"], 1)]),      # all four widths, two batches of columns
                "insert": sc.make_sdesc("insert", qc.all_words(self.w, i, ("Mark", "B16"))),
                "remove": sc.make_sdesc("remove", comps=[i["B16"], i["Mark"]]),
                "despawn": sc.make_sdesc("despawn")}

    def values(self, desc, slots, salt=1):
        return [qc.fuzz_value(slots, c, k, salt, self.w._comps[c][1]) for c, k in desc["words"]]

    def row_sets(self):
        n = self.n
        sets = {"none": [], "first": [0], "last": [n - 1], "all": range(n), "every other": range(0, n, 2), "one per unit": range(min(n - 1, 37), n, 64),
                "across a unit boundary": range(max(0, 50), min(n, 140))}
        if n > TILE: sets["across slot 8192"] = range(TILE - 70, min(n, TILE + 70))
        return {k: np.asarray(list(v), dtype=U32) for k, v in sets.items()}


_edges = {}


def edge(n):
    if n not in _edges: _edges[n] = Edge(n)
    return _edges[n]


def scatter_under_every_grid(e, desc, slots, cols, ctx):
    """From the saved state, once per launch geometry: the state after the call and the report equal the model's (so they equal each other)."""
    want, rep = sc.model_scatter(e.base, desc, slots, cols)
    try:
        for grid in GRIDS:
            e.w.handle_requests([L(0)])
            assert e.w._lib.ggrs_dbg_set_query_grid(e.w._p, grid) == 0
            got = sc.world_scatter(e.w, desc, slots, cols)
            assert got == rep, (ctx, grid, got, rep)
            sc.assert_records_equal(sc.full_record(e.w), want, f"{ctx}, grid {grid}")
    finally:
        e.w._lib.ggrs_dbg_set_query_grid(e.w._p, 0)
    return rep


@pytest.mark.parametrize("op", sc.OPS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, TILE + 77])
def test_unit_and_tile_edges(n, op):
    e = edge(n)
    e.w.handle_requests([L(0)])
    sc.assert_records_equal(sc.full_record(e.w), e.base, "the Load of frame 0 puts the world back")
    desc = e.descs()[op]
    total = {"n_dead": 0, "n_absent": 0, "n_applied": 0}
    for name, slots in e.row_sets().items():
        rep = scatter_under_every_grid(e, desc, slots, e.values(desc, slots), (n, op, name))
        assert rep["first_bad_row"] is None and rep["n_applied"] + rep["n_dead"] + rep["n_absent"] == slots.size
        for k in total: total[k] += rep[k]
    assert total["n_applied"] or n == 1
    if n >= 129: assert total["n_dead"] and (total["n_absent"] or op != "write")                     # dead slots and entities lacking the component were among the rows


def test_rows_of_one_unit_in_different_workgroups_edit_one_mask_word():
    """A dense run that starts mid-unit: rows 0..63 (one wave) are slots 30..93, rows 64..127 (the next wave) slots 94..157 -- unit 1 is edited by two waves, and
    so is every later unit; with the grid capped to 1, 2 and 7 workgroups the two waves also sit in different workgroups or in different iterations."""
    e = edge(TILE + 77)
    for op in ("insert", "remove", "despawn"):
        desc = e.descs()[op]
        slots = np.arange(30, 30 + 1000, dtype=U32)
        rep = scatter_under_every_grid(e, desc, slots, e.values(desc, slots, salt=3), ("mid-unit run", op))
        assert rep["n_applied"] > 800


# ---------------------------------------------------------------------------------------------------------------- rows that are refused
def bad_row_sets(n_rows, len_):
    """Ascending rows with one fault planted at the start, in the middle and at the last row.  A duplicate and a descending pair offend at their SECOND row (at
    the start: rows 0 and 1, first_bad_row 1); a slot at or beyond len offends at its own row (at the start: first_bad_row 0, and row 1 descends behind it)."""
    base = np.arange(3, 3 + 2 * n_rows, 2, dtype=np.int64)
    assert base[-1] < len_
    out = {}
    for where, r in (("the start", 0), ("the middle", n_rows // 2), ("the last row", n_rows - 1)):
        dup = base.copy(); desc_ = base.copy(); oob = base.copy()
        if r == 0: dup[1] = dup[0]; desc_[0], desc_[1] = base[1], base[0]                          # (a pair starts at row 0: its second row is the offender)
        else: dup[r] = dup[r - 1]; desc_[r - 1], desc_[r] = base[r], base[r - 1]
        oob[r] = len_ + (r % 3)
        out[f"a duplicate at {where}"] = dup; out[f"a descending pair at {where}"] = desc_; out[f"a slot at or beyond len at {where}"] = oob
    return out


@pytest.mark.parametrize("n_rows", [5, 700])
def test_invalid_rows_change_nothing(n_rows):
    n = 1500
    e = edge(n)
    twin = bg.World(n + 200, max_depth=4)
    build_edge(twin, n)
    e.w.handle_requests([L(0)]); twin.handle_requests([L(0)])
    seen = set()
    for op in ("write", "despawn", "insert", "remove"):
        desc = e.descs()[op]
        for name, slots in bad_row_sets(n_rows, n).items():
            want, rep = sc.model_scatter(e.base, desc, slots, e.values(desc, slots))
            assert rep["first_bad_row"] is not None
            seen.add(rep["first_bad_row"])
            for grid in (0, 2):
                assert e.w._lib.ggrs_dbg_set_query_grid(e.w._p, grid) == 0
                with pytest.raises(bg.GgrsHipError) as err:
                    e.w.scatter(slots.astype(U32), dict(zip(desc["words"], e.values(desc, slots))) or None, op=op, comps=sorted(desc["comps"]))
                assert err.value.code == bg.GGRS_E_INVALID and err.value.report.first_bad_row == rep["first_bad_row"] and f"first_bad_row {rep['first_bad_row']}" in str(err.value), (op, name, str(err.value))
            e.w._lib.ggrs_dbg_set_query_grid(e.w._p, 0)
            sc.assert_records_equal(sc.full_record(e.w), e.base, (op, name))
    assert {0, 1, n_rows // 2, n_rows - 1} <= seen
    # not a version, not a tag bit: the next Save is the twin's, which never saw the calls -- and so is what a Load of it brings back
    e.w.set_frame(0); twin.set_frame(0)
    assert e.w.handle_requests([A((0,)), S(1), A((0,))]) == twin.handle_requests([A((0,)), S(1), A((0,))])
    assert e.w.handle_requests([L(1), A((0,)), S(2)]) == twin.handle_requests([L(1), A((0,)), S(2)])
    sc.assert_records_equal(sc.full_record(e.w), sc.full_record(twin), "after the refused calls")
    twin.close()
    e.w.handle_requests([L(0)]) if e.w.has_snapshot(0) else _edges.pop(n)


# ---------------------------------------------------------------------------------------------------------------- round trips through a query
def test_query_then_scatter_of_the_untouched_result_changes_nothing():
    n = TILE + 77
    e = edge(n)
    twin = bg.World(n + 200, max_depth=4)
    build_edge(twin, n)
    e.w.handle_requests([L(0)]); twin.handle_requests([L(0)])
    i = e.ids
    r = e.w.query(bg.LIVE, [i["B64"], (i["B8"], 1), i["B16"], (i["B32"], 1)], max_rows=n + 100)    # (a buffer laid out for more rows than it holds)
    assert 0 < r.n_rows < n
    rep = e.w.scatter(r)
    assert (rep.len, rep.n_rows, rep.n_applied, rep.n_dead, rep.n_absent, rep.first_bad_row) == (n, r.n_rows, r.n_rows, 0, 0, None)
    sc.assert_records_equal(sc.full_record(e.w), e.base, "untouched result")
    e.w.set_frame(0); twin.set_frame(0)
    assert e.w.handle_requests([A((0,)), S(1)]) == twin.handle_requests([A((0,)), S(1)])
    twin.close()
    _edges.pop(n).w.close()


def test_query_edit_in_torch_scatter_query_again():
    n = 3000
    w = bg.World(n + 100, max_depth=4)
    i = build_edge(w, n)
    before = sc.full_record(w)
    fetch = [(i["B32"], 1), (i["B64"], 0), (i["B8"], 1), (i["B16"], 0)]
    r = w.query(bg.LIVE, fetch, without=[i["Mark"]])
    slots, old = r.numpy()
    r.columns[0] += 5; r.columns[1] ^= 0x0123456789ABCDEF; r.columns[2] += 200; r.columns[3] *= 3      # in place: views of the buffer
    rep = w.scatter(r)
    assert rep.n_applied == r.n_rows == slots.size and rep.n_dead == rep.n_absent == 0
    new = [old[0] + U32(5), old[1] ^ U64(0x0123456789ABCDEF), old[2] + U8(200), old[3] * U16(3)]
    want, _ = sc.model_scatter(before, sc.make_sdesc("write", fetch), slots, new)
    sc.assert_records_equal(sc.full_record(w), want, "edited in torch")
    again = w.query(bg.LIVE, fetch, without=[i["Mark"]])
    s2, c2 = again.numpy()
    assert np.array_equal(s2, slots) and all(np.array_equal(a, b) for a, b in zip(c2, new))
    # the entities of a result despawned / stripped of a component: the result's slots alone are read
    marked = w.query(bg.LIVE, [(i["B32"], 0)], with_=[i["Mark"]], max_rows=n)
    ms = marked.numpy()[0]
    state = sc.full_record(w)
    rep = w.scatter(marked, op="remove", comps=[i["B8"]])
    want, mrep = sc.model_scatter(state, sc.make_sdesc("remove", comps=[i["B8"]]), ms)
    assert rep.n_applied == mrep["n_applied"] == ms.size
    sc.assert_records_equal(sc.full_record(w), want, "remove over a result")
    rep = w.scatter(marked, op="despawn")
    want, mrep = sc.model_scatter(want, sc.make_sdesc("despawn"), ms)
    assert rep.n_applied == ms.size
    sc.assert_records_equal(sc.full_record(w), want, "despawn over a result")
    rep = w.scatter(marked)                                                                        # the entities have died since the query ran: counted, not applied
    assert (rep.n_applied, rep.n_dead, rep.n_absent) == (0, ms.size, 0)
    sc.assert_records_equal(sc.full_record(w), want, "a stale result")
    # slots and values as device tensors
    live = np.flatnonzero(sc._bits(want["alive"])[:n])[::3].astype(U32)
    vals = qc.fuzz_value(live, i["B64"], 1, 9, 8)
    rep = w.scatter(torch.from_numpy(live.astype(np.int64)).cuda(), {(i["B64"], 1): torch.from_numpy(vals.view(np.int64)).cuda()})
    want, mrep = sc.model_scatter(want, sc.make_sdesc("write", [(i["B64"], 1)]), live, [vals])
    assert rep.n_applied == mrep["n_applied"] == live.size
    sc.assert_records_equal(sc.full_record(w), want, "tensors")
    assert "scatter" in w.kernel_info()
    with pytest.raises(ValueError): w.scatter(w.query(bg.LIVE, [(i["B32"], 0)], slots=False))
    with pytest.raises(ValueError): w.scatter(live, {(i["B64"], 1): vals[:-1]})
    with pytest.raises(ValueError): w.scatter(live, {(i["B64"], 1): vals.astype(U32)})
    w.close()


# ---------------------------------------------------------------------------------------------------------------- bookkeeping: a session against the oracle
def widths_pair(n, before=None, cap=None):
    out = []
    for kind in ("lib", "oracle"):
        w = bg.World(cap or n + 64, max_depth=6) if kind == "lib" else OracleWorld(cap or n + 64, 6)
        ids = qc.build_widths(w)
        if kind == "lib" and before: before(w)
        w.set_depth(6)
        qc.spawn_widths(w, ids, n)
        for s in range(0, n, 5): w.remove_component(ids["B16"], s)
        for s in range(3, n, 17): w.despawn(s)
        out.append((w, ids))
    return out


def edit_both(pair, desc, slots, cols):
    """ONE scatter on the device world, the per-slot calls on the oracle: the reports agree."""
    (g, _), (o, _) = pair
    rep_o = sc.apply_per_slot(o, desc, slots, cols)
    rep_g = sc.world_scatter(g, desc, slots, cols)
    assert rep_g == rep_o, (rep_g, rep_o)
    return rep_g


def lists_both(pair, reqs, ids=None):
    (g, gi), (o, _) = pair
    cg, co = g.handle_requests(reqs), o.handle_requests(reqs)
    assert cg == co, (reqs, cg, co)
    cm.assert_states_equal(cm.snapshot_state(g, tuple((ids or gi).values())), cm.snapshot_state(o, tuple((ids or gi).values())), str(reqs))


def save_tick_load(pair, first, ids=None):
    """From frame `first`: a Save of the edited world, further ticks with their Saves, a Load of that Save and a resimulation, a Load of a later Save."""
    f = first
    lists_both(pair, [S(f), A((0,)), S(f + 1), A((0,)), A((0,))], ids)
    lists_both(pair, [L(f), A((0,)), S(f + 1), A((0,)), S(f + 2), A((0,))], ids)
    lists_both(pair, [L(f + 1), A((0,)), S(f + 2), A((0,))], ids)
    lists_both(pair, [L(f)], ids)
    lists_both(pair, [A((0,)), S(f + 1)], ids)


@pytest.mark.parametrize("mode", ["default", "value_tags", "lazy_live_deferred"])
def test_write_to_a_column_no_system_writes_survives_saves_and_loads(mode):
    before = {"default": None, "value_tags": lambda w: w._lib.ggrs_dbg_set_value_tags(w._p, 1), "lazy_live_deferred": lambda w: w._lib.ggrs_dbg_set_lazy_live(w._p, 3)}[mode]
    n = 2000
    pair = widths_pair(n, before)
    ids = pair[0][1]
    lists_both(pair, [S(0), A((0,)), S(1), A((0,))])                                               # every column has been saved once: its version stands
    lists_both(pair, [L(1), A((0,)), S(2), A((0,))])
    slots = np.arange(1, n, 3, dtype=U32)
    desc = sc.make_sdesc("write", [(ids["B64"], 1), (ids["B16"], 1), (ids["B8"], 0)])              # no system writes these
    rep = edit_both(pair, desc, slots, [qc.fuzz_value(slots, c, k, 4, pair[0][0]._comps[c][1]) for c, k in desc["words"]])
    assert rep["n_applied"] and rep["n_dead"] and rep["n_absent"]
    save_tick_load(pair, 3)
    # the same values again (value tags: the destination may hold them already), then other values behind a Load
    rep = edit_both(pair, desc, slots, [qc.fuzz_value(slots, c, k, 4, pair[0][0]._comps[c][1]) for c, k in desc["words"]])
    lists_both(pair, [S(4), A((0,)), S(5), A((0,))])
    lists_both(pair, [L(4)])
    edit_both(pair, desc, slots[::2], [qc.fuzz_value(slots[::2], c, k, 5, pair[0][0]._comps[c][1]) for c, k in desc["words"]])
    save_tick_load(pair, 4)
    if mode == "lazy_live_deferred": assert cm.deferred_counts(pair[0][0])[0] > 0, pair[0][0].kernel_info().get("deferred_saves")
    if mode == "value_tags": assert pair[0][0].kernel_info()["value_tags"].startswith("on")
    for w, _ in pair: w.close()


def test_insert_then_remove_of_a_component_a_system_reads():
    n = 1000
    pair = widths_pair(n)
    ids = pair[0][1]
    lists_both(pair, [S(0), A((0,)), S(1), A((0,))])
    b32 = ids["B32"]                                                                               # the world's one system adds 1 to B32.0 where the entity has it
    slots = np.arange(0, n, 2, dtype=U32)
    rep = edit_both(pair, sc.make_sdesc("remove", comps=[b32]), slots, [])
    assert rep["n_applied"] and rep["n_dead"]
    save_tick_load(pair, 2)
    back = np.arange(0, n, 4, dtype=U32)
    desc = sc.make_sdesc("insert", [(b32, 1), (b32, 0)])
    edit_both(pair, desc, back, [qc.fuzz_value(back, b32, k, 6, 4) for _, k in desc["words"]])
    save_tick_load(pair, 3)
    both = sc.make_sdesc("insert", qc.all_words(pair[0][0], ids, ("Mark", "B16")))
    edit_both(pair, both, slots, [qc.fuzz_value(slots, c, k, 7, pair[0][0]._comps[c][1]) for c, k in both["words"]])
    save_tick_load(pair, 4)
    for w, _ in pair: w.close()


def test_despawn_of_half_the_world():
    n = 3000
    pair = widths_pair(n)
    lists_both(pair, [S(0), A((0,)), S(1), A((0,))])
    slots = np.arange(1, n, 2, dtype=U32)
    rep = edit_both(pair, sc.make_sdesc("despawn"), slots, [])
    assert rep["n_applied"] > n // 3 and rep["n_dead"]
    assert pair[0][0].active_count() == pair[1][0].active_count()
    save_tick_load(pair, 2)
    lists_both(pair, [L(1), A((0,)), S(2)])                                                        # back before the despawns: everybody is there again
    assert pair[0][0].active_count() == pair[1][0].active_count() > n // 2
    for w, _ in pair: w.close()


def test_scatter_behind_an_enqueued_list():
    n = 2000
    pair = widths_pair(n)
    (g, ids), (o, _) = pair
    lists_both(pair, [S(0), A((0,)), S(1), A((0,))])
    reqs = [L(1), A((0,)), S(2), A((0,)), S(3), A((0,))]
    want = o.handle_requests(reqs)
    g.enqueue_requests(reqs)                                                                       # uncollected: the scatter is ordered behind it on the world's stream
    slots = np.arange(0, n, 3, dtype=U32)
    desc = sc.make_sdesc("write", [(ids["B32"], 0), (ids["B64"], 0)])
    cols = [qc.fuzz_value(slots, c, k, 8, g._comps[c][1]) for c, k in desc["words"]]
    rep_g = sc.world_scatter(g, desc, slots, cols)
    assert g.pending_batches() == 1
    assert g.collect_checksums() == want
    assert rep_g == sc.apply_per_slot(o, desc, slots, cols)
    save_tick_load(pair, 4)
    for w, _ in pair: w.close()


def test_component_under_a_strategy():
    import test_gpu_round5 as r5
    n = 500
    pair = []
    for kind in ("lib", "oracle"):
        w = bg.World(n + 64, max_depth=6) if kind == "lib" else OracleWorld(n + 64, 6)
        Acc, Cnt = r5._f16_world(w, True)
        w.set_depth(6)
        rng = np.random.default_rng(5)
        w.spawn(n, {Acc: [(rng.integers(-40, 40, n) * 0.5).astype(np.float32).view(U32), rng.uniform(1, 2, n).astype(np.float32).view(U32), rng.uniform(-1000, 1000, n).astype(np.float32).view(U32)],
                    Cnt: [np.zeros(n, dtype=U32)]})
        for s in range(0, n, 9): w.despawn(s)
        pair.append((w, {"Accel": Acc, "Count": Cnt}))
    ids = pair[0][1]
    lists_both(pair, [S(0), A((0,)), S(1), A((0,))])
    slots = np.arange(0, n, 2, dtype=U32)
    desc = sc.make_sdesc("write", [(ids["Accel"], 2), (ids["Accel"], 0)])                          # the live form is plain f32: served; a Save stores them as f16
    vals = [np.random.default_rng(k).uniform(-900, 900, slots.size).astype(np.float32).view(U32) for k in (1, 2)]
    rep = edit_both(pair, desc, slots, vals)
    assert rep["n_applied"] and rep["n_dead"]
    save_tick_load(pair, 2)
    for w, _ in pair: w.close()


def test_no_rollback_component_and_rollback_despawned_markers():
    import test_despawn_rollback as tdr
    n = 300
    pair = []
    for kind in ("lib", "oracle"):
        w = bg.World(n + 50, max_depth=8) if kind == "lib" else OracleWorld(n + 50, 8)
        H, M = tdr.build(w, n)
        w.set_depth(8); w.set_confirmed(0)
        pair.append((w, {"Health": H, "Mesh": M}))
    ids = pair[0][1]
    lists_both(pair, [S(0), A((0,)), A((0,)), A((0,)), S(3)])                                      # health 1, 2, 3 die in unconfirmed frames: marked RollbackDespawned, not freed
    g = pair[0][0]
    assert g.disabled_mask(n).sum() > 0
    slots = np.arange(0, n, dtype=U32)
    desc = sc.make_sdesc("write", [(ids["Mesh"], 1), (ids["Health"], 0), (ids["Mesh"], 0)])        # Mesh is live-only (GGRS_COMP_NO_ROLLBACK): served
    cols = [qc.fuzz_value(slots, ids["Mesh"], 1, 3, 4), (U32(20) + slots % U32(7)).astype(U32), qc.fuzz_value(slots, ids["Mesh"], 0, 3, 4)]
    rep = edit_both(pair, desc, slots, cols)
    assert rep["n_dead"] == int(g.disabled_mask(n).sum()) and rep["n_applied"] == n - rep["n_dead"]   # a marked entity counts as dead
    for reqs in ([A((0,)), S(4), A((0,))], [L(3), A((0,)), S(4), A((0,))], [L(4)], [L(0)]):
        lists_both(pair, reqs)
        for w, i in pair: assert w.disabled_mask(n).tolist() == pair[1][0].disabled_mask(n).tolist()
    for w, _ in pair: w.close()


def test_device_spawn_world_with_uncollected_batches_is_refused():
    import device_spawn_script as ds
    scr = ds.fans_across_empty_tiles()
    w = bg.World(scr.capacity, max_depth=scr.max_depth)
    ids = ds.build(w, scr)
    lists = [step[1] for step in scr.steps if step[0] == "list"]
    w.handle_requests(lists[0])
    plan = ids[0]
    slots = np.arange(0, min(w.len, 40), dtype=U32)
    desc = sc.make_sdesc("write", [(plan, 2)])
    cols = [np.full(slots.size, 0, dtype=U32)]
    w.enqueue_requests(lists[1])
    try:
        with pytest.raises(bg.GgrsHipError) as e: sc.world_scatter(w, desc, slots, cols)
        assert e.value.code == bg.GGRS_E_INVALID and "spawn on the device" in str(e.value) and "uncollected" in str(e.value)
    finally:
        w.collect_checksums()
    before = sc.full_record(w)
    rep = sc.world_scatter(w, desc, slots, cols)                                                   # with nothing in flight its len is known: served
    want, mrep = sc.model_scatter(before, desc, slots, cols)
    assert rep == mrep and rep["len"] == w.len
    sc.assert_records_equal(sc.full_record(w), want, "device-spawn world")
    w.close()


def test_refusals_on_a_device_world():
    e = edge(65)
    w, i = e.w, e.ids
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    rep = _ffi.ScatterReport()
    d = w.scatter_desc("write", [(i["B32"], 0), (i["B32"], 0)])
    assert w._lib.ggrs_hip_scatter(w._p, C.byref(d), buf.data_ptr(), 4, 4, C.byref(rep)) == bg.GGRS_E_INVALID and b"both name word 0 of component B32" in w._lib.ggrs_hip_last_error(w._p)
    d = w.scatter_desc("despawn")
    assert w._lib.ggrs_hip_scatter(w._p, C.byref(d), None, 0, 0, C.byref(rep)) == 0                 # no rows: a no-op that fills the report
    assert (rep.len, rep.n_rows, rep.n_applied, rep.n_dead, rep.n_absent, rep.first_bad_row) == (65, 0, 0, 0, 0, 2**64 - 1)
    assert w._lib.ggrs_hip_scatter(w._p, C.byref(d), buf.data_ptr(), 4, 5, C.byref(rep)) == bg.GGRS_E_INVALID and b"laid out for 4" in w._lib.ggrs_hip_last_error(w._p)
    e.w.handle_requests([L(0)])
    sc.assert_records_equal(sc.full_record(w), e.base, "after the refusals")
