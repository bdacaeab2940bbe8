"""The sorted query (ggrs_hip_query_sorted / ggrs_hip_query_sorted_block through World.query_sorted) against the numpy model of its semantics
(tests/sorted_query_common.py).  Every comparison is the device's whole output buffer -- pre-filled with 0xA5 -- against the model's rows laid out as the header
says, bit for bit: the rows, the bytes beyond row n_rows of every column and the padding between columns.  The widths world carries values planted for the
purpose (sorted_query_common.planted_columns): NaNs of both signs with different payloads, +-0, +-inf, denormals, integers across the sign, columns of 3 and 5
distinct values.  Wherever n_matched <= 2048 both forms -- one workgroup in one launch, and the radix launches -- run on the same input and must write the same
bytes."""
import numpy as np
import pytest
import torch

import bevy_ggrs_amd as bg
import common as cm
import query_common as qc
import sorted_query_common as sq

pytestmark = pytest.mark.gpu

U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
S, L, A = bg.SaveGameState, bg.LoadGameState, bg.AdvanceFrame
LENS = [1, 63, 64, 65, 2047, 2048, 2049, 8300]
SMALL_MAX = 2048                                             # IX_TILE: at most this many matches take the one-launch form


def mark_value(s): return ((np.asarray(s, dtype=np.int64) * 2654435761 >> 7) & 0x3FF).astype(U32)


class Planted:
    """n entities with the planted words; Mark (a u32 of few distinct values) on every third slot; liveness "all", or "sparse": about 3 % alive."""

    def __init__(self, n, liveness):
        self.n = n
        self.w = w = bg.World(n + 200, max_depth=4)
        self.ids = ids = qc.build_widths(w)
        w.set_depth(4)
        sq.spawn_planted(w, ids, n)
        marked = np.arange(0, n, 3)
        w.scatter(marked, {(ids["Mark"], 0): mark_value(marked)}, op="insert")
        if liveness == "sparse":
            keep = np.random.default_rng([5, n]).random(n) < 0.03
            keep[n - 1] = True                                                                     # (never an empty world: the last slot lives)
            if not keep.all(): w.scatter(np.flatnonzero(~keep), op="despawn")
        self.rec = qc.record(w)
        assert self.rec["len"] == n

    def set_form(self, form): assert self.w._lib.ggrs_dbg_set_sort_form(self.w._p, form) == 0

    def check(self, desc, order_by, max_rows=None, ctx="", state=bg.LIVE):
        """Both forms where the small one applies (byte-identical), each against the model; returns the model's result."""
        cap = self.n if max_rows is None else max_rows
        try:
            self.set_form(1)
            want, large = sq.assert_sorted_equals_model(self.w, state, self.rec, desc, order_by, cap, ctx=(self.n, ctx, "large form"))
            self.set_form(0)
            _, by_size = sq.assert_sorted_equals_model(self.w, state, self.rec, desc, order_by, cap, ctx=(self.n, ctx, "by size"))
            assert np.array_equal(large, by_size), (self.n, ctx)
        finally:
            self.set_form(0)
        return want


_worlds = {}


def planted(n, liveness="all"):
    if (n, liveness) not in _worlds: _worlds[(n, liveness)] = Planted(n, liveness)
    return _worlds[(n, liveness)]


def key_configs(i):
    """Every kind at every width it allows, DESC, and 2 and 4 keys mixing widths."""
    B8, B16, B32, B64 = i["B8"], i["B16"], i["B32"], i["B64"]
    single = [(B8, 0, "u"), (B8, 0, "i"), (B16, 0, "u"), (B16, 0, "i"), (B32, 1, "u"), (B32, 1, "i"), (B32, 0, "f"), (B64, 1, "u"), (B64, 1, "i"), (B64, 0, "f"),
              (B8, 1, "u", "desc"), (B16, 2, "i", "desc"), (B32, 0, "f", "desc"), (B64, 0, "f", "desc"), (B64, 1, "i", "desc")]
    multi = [[(B8, 1, "u"), (B32, 0, "f", "desc")], [(B16, 2, "u", "desc"), (B64, 1, "i")], [(B8, 1, "u"), (B16, 2, "u", "desc"), (B64, 0, "f"), (B32, 1, "i")]]
    return [[k] for k in single] + multi


def fetch_all(p):
    i = p.ids
    return [(i["B64"], 1), (i["B8"], 0), (i["B32"], 0), (i["B16"], 2), (i["B8"], 1), (i["B64"], 0)]


@pytest.mark.parametrize("liveness", ["all", "sparse"])
@pytest.mark.parametrize("n", LENS)
def test_every_len_liveness_and_key(n, liveness):
    p = planted(n, liveness)
    desc = qc.make_desc(fetch_all(p))
    alive = int(qc.as_bits(p.rec["alive"], n).sum())
    assert alive == n if liveness == "all" else 1 <= alive <= max(1, n // 8)
    for order_by in key_configs(p.ids):
        want = p.check(desc, order_by, ctx=order_by)
        assert want["n_matched"] == alive
    # nobody matches: everyone has B16
    want = p.check(qc.make_desc([(p.ids["B8"], 0), (p.ids["B64"], 1)], without=[p.ids["B16"]]), [(p.ids["B32"], 0, "f")], ctx="nobody")
    assert want["n_matched"] == 0


@pytest.mark.parametrize("n", [65, 2049, 8300])
def test_max_rows_is_a_top_k_and_nothing_beyond_it_is_written(n):
    p = planted(n)
    i = p.ids
    desc = qc.make_desc(fetch_all(p))
    for order_by in ([(i["B64"], 0, "f", "desc")], [(i["B8"], 1, "u"), (i["B32"], 1, "i")]):
        full = sq.model_query_sorted(p.rec, desc, order_by, n)
        for cap in (0, 1, 37, n + 64):                                                             # a count; one row; a cut inside the first 64 rows; room to spare
            want = p.check(desc, order_by, cap, ctx=(order_by, cap))
            assert want["n_matched"] == n and want["n_rows"] == min(cap, n) and want["slots"].tolist() == full["slots"][:cap].tolist()
    p.check(qc.make_desc([], slots=True), [(i["B16"], 0, "i")], 37, ctx="slots only")
    p.check(qc.make_desc([(i["B8"], 0)], slots=False), [(i["B16"], 0, "i")], 37, ctx="no slots")
    want = p.check(qc.make_desc([], slots=False), [(i["B16"], 0, "i")], 37, ctx="nothing written")
    assert want["n_matched"] == n


@pytest.mark.parametrize("n, liveness", [(2049, "all"), (8300, "all"), (8300, "sparse")])
def test_launch_geometry_does_not_change_a_byte(n, liveness):
    p = planted(n, liveness)
    i = p.ids
    desc = qc.make_desc(fetch_all(p))
    try:
        for order_by, cap in (([(i["B8"], 1, "u", "desc"), (i["B64"], 0, "f")], n), ([(i["B32"], 0, "f")], 100)):
            runs = []
            for grid in (0, 1, 2, 7, 0):                                                           # by size, capped to 1, 2 and 7 workgroups, by size again
                assert p.w._lib.ggrs_dbg_set_query_grid(p.w._p, grid) == 0
                for form in (0, 1):
                    p.set_form(form)
                    runs.append(sq.device_query_sorted(p.w, bg.LIVE, desc, order_by, cap))
                p.check(desc, order_by, cap, ctx=f"grid {grid}")
            for r in runs[1:]: assert r[:2] == runs[0][:2] and np.array_equal(r[2], runs[0][2])
    finally:
        p.w._lib.ggrs_dbg_set_query_grid(p.w._p, 0); p.set_form(0)


def test_two_consecutive_calls_and_a_key_that_is_not_fetched():
    p = planted(2049)
    i = p.ids
    order_by = [(i["B16"], 2, "u"), (i["B32"], 0, "f", "desc")]
    desc = qc.make_desc([(i["B64"], 1), (i["B8"], 0)])                                             # neither key word is fetched
    a = sq.device_query_sorted(p.w, bg.LIVE, desc, order_by, p.n)
    b = sq.device_query_sorted(p.w, bg.LIVE, desc, order_by, p.n)
    assert a[:2] == b[:2] and np.array_equal(a[2], b[2])
    p.check(desc, order_by, ctx="keys not fetched")
    # a key's component counts as With: Mark sits on every third slot
    want = p.check(desc, [(i["Mark"], 0, "u")], ctx="an implied With")
    assert want["n_matched"] == len(range(0, p.n, 3)) and (want["slots"] % 3 == 0).all()
    # the result's views
    r = p.w.query_sorted(bg.LIVE, [(i["B32"], 0)], [(i["B32"], 0, "f")], max_rows=10)
    full = sq.model_query_sorted(p.rec, qc.make_desc([(i["B32"], 0)]), [(i["B32"], 0, "f")], 10)
    slots, cols = r.numpy()
    assert (r.n_matched, r.n_rows, r.len) == (p.n, 10, p.n) and np.array_equal(slots, full["slots"]) and np.array_equal(cols[0], full["columns"][0])
    assert r.columns[0].dtype == torch.int32 and r.words == [(i["B32"], 0)]


def test_a_key_on_a_component_the_host_toggles():
    p = Planted(300, "all")
    w, i = p.w, p.ids
    desc, order_by = qc.make_desc([(i["Mark"], 0), (i["B8"], 0)]), [(i["Mark"], 0, "u", "desc"), (i["B8"], 0, "i")]
    before = p.check(desc, order_by, ctx="as planted")
    for s in (0, 3, 150, 297): w.remove_component(i["Mark"], s)
    for s, v in ((1, 5), (2, 5), (299, 0x3FF), (64, 0)): w.insert_component(i["Mark"], s, np.array([v], dtype=U32))
    p.rec = qc.record(w)
    after = p.check(desc, order_by, ctx="toggled")
    assert after["n_matched"] == before["n_matched"] and set(after["slots"].tolist()) == (set(before["slots"].tolist()) - {0, 3, 150, 297}) | {1, 2, 299, 64}
    w.close()


# ---------------------------------------------------------------------------------------------------------------- sides: ring frames, LIVE, a block
def test_synctest_session_every_ring_frame_a_block_and_live():
    n = 2500
    w = bg.World(n + 200, max_depth=8)
    ids = qc.build_widths(w)
    sq.spawn_planted(w, ids, n)
    w.scatter(np.arange(5, n, 9), op="despawn")                                                    # dead slots below len
    drv = cm.SyncTestDriver(w, 3)
    for t in range(9): drv.tick((0,))                                                              # the frames differ in B32.0: the system adds 1 to its bits
    frames = [f for f in range(w.frame + 1, w.frame - 40, -1) if w.has_snapshot(f)]
    assert len(frames) >= 3
    desc = qc.make_desc([(ids["B32"], 0), (ids["B64"], 1), (ids["B8"], 1)])
    orders = ([(ids["B32"], 0, "f")], [(ids["B8"], 1, "u", "desc"), (ids["B64"], 0, "f")])
    cap = n + 64
    live = qc.record(w)
    for order_by in orders: sq.assert_sorted_equals_model(w, bg.LIVE, live, desc, order_by, cap, ctx=("LIVE", order_by))
    got = {}
    for f in frames:
        blk = w.snapshot_copy(f)
        for k, order_by in enumerate(orders):
            got[(f, k)] = sq.device_query_sorted(w, f, desc, order_by, cap)
            via_block = sq.device_query_sorted(w, blk, desc, order_by, cap)
            assert via_block[:2] == got[(f, k)][:2] and np.array_equal(via_block[2], got[(f, k)][2]), (f, order_by)
    assert not np.array_equal(got[(frames[0], 0)][2], got[(frames[-1], 0)][2])
    for f in frames:                                                                              # (a Load drops the frames behind it: newest first)
        w.handle_requests([L(f)])
        rec = qc.record(w)
        for k, order_by in enumerate(orders):
            want = sq.model_query_sorted(rec, desc, order_by, cap)
            n_matched, n_rows, buf = got[(f, k)]
            assert (n_matched, n_rows) == (want["n_matched"], want["n_rows"]), (f, order_by)
            assert np.array_equal(buf, sq.expected_buffer(want, qc.word_bytes_of(w, desc), cap, buf.size)), (f, order_by)
            assert n_matched == n - len(range(5, n, 9))
    with pytest.raises(bg.GgrsHipError) as e: w.query_sorted(999, [], orders[0])
    assert e.value.code == bg.GGRS_E_NO_SNAPSHOT
    w.close()


STRATEGY_SRC = ("__device__ void ggrs_store(const GgrsWords& t, GgrsWords& s) { s.u16(0) = (unsigned short)t.u32(0); }\n"
                "__device__ void ggrs_load(const GgrsWords& s, GgrsWords& t) { t.u32(0) = s.u16(0); }")


def test_a_strategy_component_key_is_served_on_live_and_refused_on_a_frame():
    w = bg.World(200, max_depth=4)
    Al = w.register_component("Alpha", 4, 1); Be = w.register_component("Beta", 4, 1)
    w.checksum_component(Al, [0]); w.checksum_component(Be, [0])
    w.register_component_strategy(Al, 2, 1, STRATEGY_SRC)
    w.add_system(bg.SYS_ADD_U32, comp=(Be,), word=(0,), iparam=(1,))
    w.set_depth(4)
    w.spawn(100, {Al: [(np.arange(100, dtype=U32) * 37) % 11], Be: [np.arange(100, dtype=U32) * 3]})
    for s in range(0, 100, 4): w.remove_component(Al, s)
    w.handle_requests([S(0), A((0,)), S(1), A((0,))])
    rec = qc.record(w)
    desc = qc.make_desc([(Be, 0)])
    want, _ = sq.assert_sorted_equals_model(w, bg.LIVE, rec, desc, [(Al, 0, "u", "desc")], 100, ctx="LIVE: live-form words are served")
    assert want["n_matched"] == 75
    for state in (1, w.snapshot_copy(1)):
        with pytest.raises(bg.GgrsHipError) as e: sq.device_query_sorted(w, state, desc, [(Al, 0, "u")], 100)
        assert e.value.code == bg.GGRS_E_INVALID and "Strategy" in str(e.value) and "sort key 0" in str(e.value)
    got = sq.device_query_sorted(w, 1, qc.make_desc([(Be, 0)], with_=[Al]), [(Be, 0, "u", "desc")], 100)      # filtering on its presence in a frame is served
    w.handle_requests([L(1)])
    want = sq.model_query_sorted(qc.record(w), qc.make_desc([(Be, 0)], with_=[Al]), [(Be, 0, "u", "desc")], 100)
    assert got[:2] == (want["n_matched"], want["n_rows"]) == (75, 75) and np.array_equal(got[2], sq.expected_buffer(want, [4], 100, got[2].size))
    w.close()


def test_scatter_refuses_a_sorted_result_and_the_world_is_unchanged():
    p = Planted(500, "all")
    w, i = p.w, p.ids
    r = w.query_sorted(bg.LIVE, [(i["B32"], 1)], [(i["B32"], 1, "i")])
    slots = r.numpy()[0].astype(np.int64)
    first_bad = int(np.flatnonzero(slots[1:] <= slots[:-1])[0]) + 1                               # the first row whose slot does not ascend
    r.columns[0].zero_()                                                                           # values that WOULD change the world
    with pytest.raises(bg.GgrsHipError) as e: w.scatter(r, op="write")
    assert e.value.code == bg.GGRS_E_INVALID and e.value.report.first_bad_row == first_bad
    after = qc.record(w)
    assert np.array_equal(qc.as_bits(after["alive"], p.n), qc.as_bits(p.rec["alive"], p.n))
    for key, col in p.rec["columns"].items(): assert np.array_equal(after["columns"][key], col), key
    w.close()
