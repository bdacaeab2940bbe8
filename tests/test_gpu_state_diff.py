"""The device state diff (ggrs_hip_diff_frames / ggrs_hip_diff_block / ggrs_hip_snapshot_copy) against the numpy model of its semantics
(tests/state_diff_common.py), at the wave-unit (64) and layout-tile (8192) edges.  One world per size runs ONE script of Saves with host edits between them; every
Save's arrays are recorded through the download calls, every frame stays in the ring, and the tests compare pairs of frames."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import bevy_ggrs_amd as bg
import common as cm
import state_diff_common as sd
from bevy_ggrs_amd import _ffi

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 8191, 8192, 8193, 2 * 8192 + 5]
U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
LABELS = ["s0", "same", "advanced", "uploads", "structure", "entities", "resource", "planted_a", "planted_b"]


class Scenario:
    def __init__(self, n, vtags=False):
        self.n = n
        self.w = w = bg.World(n + 70, max_depth=12)
        self.s = s = sd.build_schema(w)
        if vtags: assert w._lib.ggrs_dbg_set_value_tags(w._p, 1) == 0
        w.set_depth(12)
        sd.spawn_schema(w, s, n)
        if vtags: assert w.kernel_info()["value_tags"].startswith("on"), w.kernel_info()["value_tags"]
        self.frames, self.recs = {}, {}
        ids, at = s.ids, lambda k: k % n
        self._f = 0
        self.snap("s0")
        self.snap("same")                                                      # two Saves with nothing between them
        w.handle_requests([sd.adv(1)]); self.snap("advanced")                  # one Advance apart
        # upload_word on every word width
        w.upload_word(ids["Flag"], 0, at(2), np.array([200], dtype=U8)); w.upload_word(ids["Tag"], 0, at(8), np.array([65000], dtype=U16))
        w.upload_word(ids["Pos"], 1, at(63), np.array([0x80000000], dtype=U32)); w.upload_word(ids["Big"], 0, at(64), np.array([(1 << 63) | 5], dtype=U64))
        w.upload_word(ids["Quiet"], 0, at(8191), np.array([4242], dtype=U32)); w.upload_word(ids["Pos"], 0, at(8192), np.array([1], dtype=U32))
        self.snap("uploads")
        w.insert_component(ids["Quiet"], 0, np.array([99], dtype=U32)); w.remove_component(ids["Tag"], at(1)); w.remove_component(ids["Pos"], at(9))
        self.snap("structure")
        w.despawn(at(n // 2)); w.despawn(at(66))
        i = np.arange(3)
        w.spawn(3, {ids["Flag"]: [i.astype(U8)], ids["Pos"]: [(i + 5).astype(U32), (i + 6).astype(U32)], ids["Big"]: [(i + 7).astype(U64)], ids["Side"]: [i.astype(U32)]})
        self.snap("entities")
        w.resource_write(s.clock, [1000, 77]); self.snap("resource")
        # a value planted under a slot that is then despawned, and under a removed component: not state
        p, q = at(3), at(10)
        w.upload_word(ids["Quiet"], 0, p, np.array([1111], dtype=U32)); w.despawn(p); w.remove_component(ids["Big"], q)
        self.snap("planted_a")
        w.upload_word(ids["Quiet"], 0, p, np.array([2222], dtype=U32)); w.upload_word(ids["Big"], 0, q, np.array([3333], dtype=U64))
        w.upload_word(ids["Side"], 0, 0, np.array([777], dtype=U32))           # a non-rollback component: ignored
        self.snap("planted_b")

    def snap(self, label):
        self.w.set_frame(self._f)
        self.recs[label] = sd.record(self.w, self.s)
        self.w.save()
        self.frames[label] = self._f
        self._f += 1

    def model(self, a, b, cap=64): return sd.model_diff(self.recs[a], self.recs[b], self.s.comps, cap)

    def device(self, a, b, cap=64, **kw): return sd.as_model(self.w.diff(self.frames[a], self.frames[b], max_entries=cap, **kw))


_cache = {}


def scenario(n, vtags=False):
    if (n, vtags) not in _cache: _cache[(n, vtags)] = Scenario(n, vtags)
    return _cache[(n, vtags)]


@pytest.mark.parametrize("n", SIZES)
def test_every_pair_of_saves_matches_the_model(n):
    sc = scenario(n)
    assert all(sc.w.has_snapshot(f) for f in sc.frames.values())
    for a, b in itertools.combinations(LABELS, 2):
        want = sc.model(a, b)
        assert sc.device(a, b) == want, (a, b)
        assert sc.device(a, b, trust_versions=True) == want, (a, b, "trust_versions")
    # what the script was written to show
    assert sc.model("s0", "same")["n_entities"] == 0 and not sc.w.diff(sc.frames["s0"], sc.frames["same"])
    adv = sc.model("same", "advanced")
    assert adv["n_entities"] == n and adv["n_value"] == {sc.s.ids["Pos"]: n, sc.s.ids["Big"]: n} and adv["resource_diff"] == [sc.s.clock]
    assert sc.model("uploads", "structure")["n_presence"] != {} and sc.model("structure", "entities")["n_alive"] >= 3
    assert sc.model("entities", "resource") == dict(sc.model("entities", "entities"), resource_diff=[sc.s.clock])
    assert sc.model("planted_a", "planted_b")["n_entities"] == 0 and sc.device("planted_a", "planted_b")["n_entities"] == 0


@pytest.mark.parametrize("n", SIZES)
def test_live_world_against_frames(n):
    sc = scenario(n)
    last = LABELS[-1]
    assert not sc.w.diff(bg.LIVE, sc.frames[last]) and not sc.w.diff(sc.frames[last], bg.LIVE, trust_versions=True)
    got = sd.as_model(sc.w.diff(bg.LIVE, sc.frames["s0"]))
    assert got == sc.model(last, "s0")
    assert sd.as_model(sc.w.diff(sc.frames["s0"], bg.LIVE, trust_versions=True)) == sc.model("s0", last)


@pytest.mark.parametrize("n", SIZES)
def test_max_entries_order_and_geometry(n):
    sc = scenario(n)
    a, b = "s0", "planted_b"
    total = sc.model(a, b)["n_entities"]
    assert total >= 1
    for cap in (0, 1, total, total + 5):
        want = sc.model(a, b, cap)
        assert len(want["entries"]) == min(cap, total)
        runs = []
        for grid in (0, 1, 3, 0):                                              # by size, one workgroup, three, and by size again: the same report
            assert sc.w._lib.ggrs_dbg_set_diff_grid(sc.w._p, grid) == 0
            runs.append(sc.device(a, b, cap))
        assert all(r == want for r in runs), cap
        slots = [e[0] for e in runs[0]["entries"]]
        assert slots == sorted(slots) and len(set(slots)) == len(slots)


def test_counts_without_entries_through_the_c_abi():
    sc = scenario(65)
    rep = _ffi.DiffReport()
    assert sc.w._lib.ggrs_hip_diff_frames(sc.w._p, sc.frames["same"], sc.frames["advanced"], 0, C.byref(rep), None, 0) == 0
    assert rep.n_entities == 65 and rep.n_entries == 0 and rep.len_a == rep.len_b == 65


@pytest.mark.parametrize("n", [65, 8193])
def test_value_tags_forced_on_give_the_same_report(n):
    on, off = scenario(n, vtags=True), scenario(n)
    for a, b in itertools.combinations(LABELS, 2):
        assert on.device(a, b) == off.device(a, b) == on.model(a, b), (a, b)
        assert on.device(a, b, trust_versions=True) == on.model(a, b), (a, b)


@pytest.mark.parametrize("n", [63, 8193])
def test_snapshot_copy_and_diff_block(n):
    sc = scenario(n)
    w, f = sc.w, sc.frames["uploads"]
    blk = w.snapshot_copy(f)
    assert blk.dtype == torch.uint8 and blk.numel() == w.state_bytes() and blk.is_cuda
    assert not w.diff(f, blk) and not w.diff(blk, f)
    assert sd.as_model(w.diff(sc.frames["advanced"], blk)) == sc.model("advanced", "uploads")
    assert sd.as_model(w.diff(blk, sc.frames["entities"])) == sc.model("uploads", "entities")          # the tensor as side A: the report the other way round
    assert sd.as_model(w.diff(bg.LIVE, blk)) == sc.model(LABELS[-1], "uploads")
    with pytest.raises(bg.GgrsHipError) as e: w.diff(f, blk, trust_versions=True)
    assert e.value.code == bg.GGRS_E_INVALID and "row versions" in str(e.value)


def test_diff_block_against_an_edited_copy():
    """Runs last on its world: a handed-out column pointer tells where a word lies inside a block (and ends the world's row-version shortcuts for that column)."""
    sc = Scenario(8193)
    w, s = sc.w, sc.s
    blk = w.snapshot_copy(sc.frames["uploads"])
    live = w.live_state_ptr()
    rec = dict(sc.recs["uploads"]); rec["words"] = {k: v.copy() for k, v in rec["words"].items()}
    for name, word, slot, val, dt in (("Pos", 1, 8192, 0xDEADBEEF, U32), ("Big", 0, 100, 0x0123456789ABCDEF, U64), ("Flag", 0, 8191, 0xEE, U8), ("Tag", 0, 71, 0xBEE, U16)):
        ptr, ts = w.column_device_ptr(s.ids[name], word)
        wb = np.dtype(dt).itemsize
        off = ptr - live + (slot // 8192) * ts + (slot % 8192) * wb
        blk[off:off + wb] = torch.from_numpy(np.array([val], dtype=dt).view(U8).copy()).to(blk.device)
        rec["words"][(s.ids[name], word)][slot] = val
    want = sd.model_diff(sc.recs["uploads"], rec, s.comps)
    assert want["n_entities"] == 4 and len(want["n_value"]) == 4
    assert sd.as_model(w.diff(sc.frames["uploads"], blk)) == want
    w.close()


def test_refusals():
    sc = scenario(64)
    w = sc.w
    with pytest.raises(bg.GgrsHipError) as e: w.diff(sc.frames["s0"], 999)
    assert e.value.code == bg.GGRS_E_NO_SNAPSHOT
    with pytest.raises(bg.GgrsHipError) as e: w.snapshot_copy(999)
    assert e.value.code == bg.GGRS_E_NO_SNAPSHOT
    # outstanding batches: refused as the other synchronous calls are
    w.set_frame(sc._f); w.enqueue_requests([bg.SaveGameState(sc._f)])
    try:
        with pytest.raises(bg.GgrsHipError) as e: w.diff(sc.frames["s0"], sc.frames["same"])
        assert e.value.code == bg.GGRS_E_INVALID and "uncollected" in str(e.value)
        with pytest.raises(bg.GgrsHipError) as e: w.snapshot_copy(sc.frames["s0"])
        assert e.value.code == bg.GGRS_E_INVALID
    finally:
        w.collect_checksums()
    assert not w.diff(sc.frames["s0"], sc.frames["same"])
    # a world with a component under a Strategy: live form against Stored form is refused, frame against frame is allowed
    g = bg.World(200, max_depth=4)
    A = g.register_component("Alpha", 4, 1); B = g.register_component("Beta", 4, 1)
    g.checksum_component(A, [0]); g.checksum_component(B, [0])
    g.register_component_strategy(A, 2, 1, "__device__ void ggrs_store(const GgrsWords& t, GgrsWords& s) { s.u16(0) = (unsigned short)t.u32(0); }\n"
                                           "__device__ void ggrs_load(const GgrsWords& s, GgrsWords& t) { t.u32(0) = s.u16(0); }")
    g.add_system(bg.SYS_ADD_U32, comp=(B,), word=(0,), iparam=(1,))
    g.set_depth(4)
    g.spawn(100, {A: [np.arange(100, dtype=U32)], B: [np.arange(100, dtype=U32)]})
    g.handle_requests([bg.SaveGameState(0), bg.AdvanceFrame((0,)), bg.SaveGameState(1)])
    with pytest.raises(bg.GgrsHipError) as e: g.diff(bg.LIVE, 1)
    assert e.value.code == bg.GGRS_E_INVALID and "Strategy" in str(e.value)
    d = g.diff(0, 1)
    assert d.n_entities == 100 and d.n_value == {B: 100}                       # Alpha's Stored words are equal, Beta was advanced
    g.close()


def test_live_against_the_newest_frame_right_after_a_synctest_tick():
    """A steady SyncTest session with the lazy live block and deferred Saves forced on: the tick's last AdvanceFrame (input 0: the world's systems do nothing) is
    owed to the live block, its later Saves are owed to the ring.  The diff brings both up to date first."""
    n, cd = 8193, 3
    w = bg.World(n, max_depth=8)
    s = sd.build_schema(w, with_side=False)                                    # (a non-rollback component keeps the live block written by every tick)
    assert w._lib.ggrs_dbg_set_lazy_live(w._p, 3) == 0
    sd.spawn_schema(w, s, n)
    drv = cm.SyncTestDriver(w, cd)
    for _ in range(10): drv.tick((1,))
    drv.tick((0,))
    deferred, materialised = cm.deferred_counts(w)
    lazy0 = w.kernel_info()["lazy_live_block"]
    assert deferred > 0, w.kernel_info()["deferred_saves"]
    newest = w.frame - 1
    assert w.has_snapshot(newest) and w.has_snapshot(newest - 1)
    d = w.diff(bg.LIVE, newest)
    assert not d, str(d)
    assert cm.deferred_counts(w)[1] > materialised, w.kernel_info()["deferred_saves"]
    assert not lazy0.startswith("on") or w.kernel_info()["lazy_live_block"] != lazy0, lazy0       # (where the text carries the counts, one more was materialised)
    assert not w.diff(bg.LIVE, newest, trust_versions=True)
    # the frame before was advanced with input 1: every entity that has Pos and Big moved, the clock ticked
    alive = w.alive_mask(n); both = alive & w.present_mask(s.ids["Pos"], n) & w.present_mask(s.ids["Big"], n)
    for trust in (False, True):
        d = w.diff(newest - 1, newest, trust_versions=trust)
        assert d.n_entities == int(both.sum()) == n and d.n_value == {s.ids["Pos"]: n, s.ids["Big"]: n} and d.resource_diff == [s.clock] and d.n_alive == 0
        assert [e.slot for e in d.entries] == list(range(64)) and all(e.first_name == "Pos" and e.first_word == 0 and e.first_b - e.first_a == 3 for e in d.entries)
    assert "Pos" in str(d) and "slot 0" in str(d)
    w.close()
