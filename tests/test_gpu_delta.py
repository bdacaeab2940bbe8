"""The device delta (ggrs_hip_delta_frames / ggrs_hip_delta_block; World.delta) against the numpy model of its semantics (tests/delta_common.py).  Every
comparison is the device's whole output buffer -- pre-filled with 0xA5 -- against the model's rows laid out as the query's header section says, bit for bit: the
rows, the bytes beyond row n_rows of every column and the padding between columns.  The model's inputs are the library's own download calls, taken where the
live world IS the frame being saved."""
import ctypes as C

import numpy as np
import pytest
import torch

import bevy_ggrs_amd as bg
import common as cm
import delta_common as dc
import query_common as qc
from bevy_ggrs_amd import _ffi

pytestmark = pytest.mark.gpu

LENS = [1, 63, 64, 65, 129, 8269]                                                                  # (the last crosses the 8192-slot layout tile)
U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
S, L, A = bg.SaveGameState, bg.LoadGameState, bg.AdvanceFrame
LIVE = bg.LIVE
NEAR, FAR = 5, 70                                                                                  # how much len grows: less than a 64-slot unit, more than one


# ---------------------------------------------------------------------------------------------------------------- the scenes
class Scene:
    """Three states of one build_widths world: frame 0 (len n), frame 1 (len n + NEAR) and the live world (len n + NEAR + FAR).  Between them the host despawns,
    removes, inserts (new and again), rewrites single words -- also under slots dead on both sides and under absent components -- and spawns; every Advance adds
    1 to B32.0 of whoever has it.  rec[state]: the state through the download calls."""

    def __init__(self, n):
        self.n, self.rec = n, {}
        self.w = w = bg.World(n + 400, max_depth=4)
        self.ids = i = qc.build_widths(w)
        w.set_depth(4)
        self.step = step = 1 if n < 1000 else 8                                                    # (a big world is edited more sparsely: the host calls are one by one)
        qc.spawn_widths(w, i, n)
        for s in range(0, n, 7 * step): w.insert_component(i["Mark"], s, np.array([s ^ 0x5A5A5A], dtype=U32))
        for s in range(0, n, 11 * step): w.remove_component(i["B16"], s)
        for s in range(12, n, 13): w.despawn(s)
        self.rec[0] = qc.record(w)
        w.handle_requests([S(0)])
        self._edit(1)
        qc.spawn_widths(w, i, NEAR, first=n)
        w.handle_requests([A((0,)), S(1)])
        self.rec[1] = qc.record(w)
        self._edit(2)
        qc.spawn_widths(w, i, FAR, first=n + NEAR)
        w.insert_component(i["Mark"], n + NEAR + FAR - 1, np.array([7], dtype=U32))
        w.despawn(n + NEAR + 1)                                                                    # spawned and gone again before anybody saw it
        w.handle_requests([A((0,))])
        self.rec[LIVE] = qc.record(w)
        assert [self.rec[k]["len"] for k in (0, 1, LIVE)] == [n, n + NEAR, n + NEAR + FAR]
        self.blocks = {f: w.snapshot_copy(f) for f in (0, 1)}

    def _edit(self, k):
        w, i, n, st = self.w, self.ids, self.w.len, self.step
        alive = w.alive_mask()
        for s in range(k, n, 5 * st):
            if alive[s]: w.despawn(s)
        alive = w.alive_mask()                                                                     # (the host's single-entity calls are for living entities)
        for s in range(k + 1, n, 9 * st):
            if alive[s]: w.remove_component(i["B64"], s)
        for s in range(k + 2, n, 6 * st):
            if alive[s]: w.insert_component(i["Mark"], s, np.array([s + 1000 * k], dtype=U32))
        for s in range(k + 3, n, 10 * st):
            if alive[s]: w.insert_component(i["B16"], s, np.array([s & 0xFFFF, k, 9], dtype=U16))
        b8 = w.download_word(i["B8"], 1); b8[::4] ^= U8(0x80 >> k); w.upload_word(i["B8"], 1, 0, b8)          # every 4th slot, dead or alive
        b64 = w.download_word(i["B64"], 0); b64[12::13] += U64(k); w.upload_word(i["B64"], 0, 0, b64)           # under slots dead since before frame 0, and more

    def descs(self):
        i = self.ids
        wide = [(i["B64"], 1), (i["B8"], 0), (i["B32"], 1), (i["B16"], 2), (i["B8"], 1), (i["B64"], 0), (i["B32"], 0)]
        every = [i[nm] for nm in ("B8", "B16", "B32", "B64", "Mark")]
        return [dc.make_delta("changed", every, wide), dc.make_delta("changed", [i["B8"], i["B64"]], [(i["B32"], 1)], without=[i["Mark"]]),
                dc.make_delta("changed", [i["Mark"]], [], slots=True), dc.make_delta("changed", [i["B16"]], [(i["B16"], 0)], slots=False),
                dc.make_delta("added", [i["Mark"], i["B16"]], [(i["B8"], 0)]), dc.make_delta("added", [i["B64"]], [], with_=[i["Mark"]]),
                dc.make_delta("removed", [i["B64"], i["B16"]], [(i["B32"], 0), (i["B8"], 1)]), dc.make_delta("removed", [i["Mark"]], [(i["Mark"], 0)]),
                dc.make_delta("despawned", (), [(i["B64"], 0), (i["B16"], 1)]), dc.make_delta("despawned", (), [], with_=[i["Mark"]])]

    def state(self, key): return self.blocks[key[1]] if isinstance(key, tuple) else key

    def check(self, new, old, desc, cap, ctx="", **kw):
        rec_old = self.rec[old[1] if isinstance(old, tuple) else old]
        return dc.assert_delta_equals_model(self.w, new, self.state(old), self.rec[new], rec_old, desc, cap, ctx=(self.n, new, old, cap, ctx), **kw)


_scenes = {}


def scene(n):
    if n not in _scenes: _scenes[n] = Scene(n)
    return _scenes[n]


# frame / frame both ways, LIVE / frame, frame / LIVE, frame / block: len differing by NEAR and by NEAR + FAR, forward and backward
PAIRS = [(1, 0), (0, 1), (LIVE, 0), (0, LIVE), (LIVE, 1), (1, LIVE), (1, ("block", 0)), (0, ("block", 1)), (LIVE, ("block", 0))]
CUT = 3                                                                                            # a max_rows inside the first 64-slot unit


@pytest.mark.parametrize("n", LENS)
def test_every_kind_side_and_max_rows(n):
    sc = scene(n)
    seen = {k: 0 for k in dc.KINDS}
    beyond = 0
    for new, old in PAIRS:
        for desc in sc.descs():
            for cap in (n + NEAR + FAR + 64, CUT, 0):                                               # everything, a cut inside the first unit, a count
                want = sc.check(new, old, desc, cap)
                assert want["n_rows"] == min(want["n_matched"], cap)
            seen[desc["kind"]] += want["n_matched"]
            beyond += want["n_beyond_old_len"]
    assert all(seen.values()) and beyond > 0, (seen, beyond)                                      # no kind was only ever empty; some rows lay beyond old's len
    if n >= 63:
        first = dc.model_delta(sc.rec[1], sc.rec[0], sc.descs()[0], n)["all_slots"]
        assert (first < 64).sum() > CUT                                                            # CUT did fall inside the first unit


@pytest.mark.parametrize("n", LENS)
def test_launch_geometry_does_not_change_a_byte(n):
    sc = scene(n)
    try:
        for new, old in ((1, 0), (0, LIVE), (LIVE, ("block", 1))):
            for desc in sc.descs():
                for cap in (n + NEAR + FAR + 64, CUT):
                    runs = []
                    for grid in (0, 1, 2, 7):                                                      # by size, capped to 1, 2 and 7 workgroups
                        assert sc.w._lib.ggrs_dbg_set_query_grid(sc.w._p, grid) == 0
                        runs.append(dc.device_delta(sc.w, new, sc.state(old), desc, cap))
                    sc.check(new, old, desc, cap, ctx="grid 7")
                    for r in runs[1:]: assert r[0] == runs[0][0] and np.array_equal(r[1], runs[0][1])
    finally:
        sc.w._lib.ggrs_dbg_set_query_grid(sc.w._p, 0)
    assert "delta" in sc.w.kernel_info()


@pytest.mark.parametrize("n", [65, 8269])
def test_trust_versions_gives_the_same_bytes(n):
    sc = scene(n)
    for new, old in ((1, 0), (0, 1), (LIVE, 0), (1, LIVE)):
        for desc in sc.descs():
            cap = n + NEAR + FAR + 64
            plain = dc.device_delta(sc.w, new, old, desc, cap)
            trusted = dc.device_delta(sc.w, new, old, desc, cap, trust_versions=True)
            assert plain[0] == trusted[0] and np.array_equal(plain[1], trusted[1]), (new, old, desc)
            sc.check(new, old, desc, cap, ctx="trusted", trust_versions=True)
    with pytest.raises(bg.GgrsHipError) as e: dc.device_delta(sc.w, 1, sc.blocks[0], sc.descs()[0], 10, trust_versions=True)
    assert e.value.code == bg.GGRS_E_INVALID and "foreign block" in str(e.value)


def test_trust_versions_skips_the_words_nobody_wrote():
    """Two Saves with one Advance between them: the world's one system writes B32.0, so every other column carries the same version in both frames."""
    w = bg.World(600, max_depth=4)
    i = qc.build_widths(w)
    w.set_depth(4)
    qc.spawn_widths(w, i, 300)
    w.handle_requests([S(0), A((0,)), S(1)])
    rec1 = qc.record(w)
    w.handle_requests([L(0)]); rec0 = qc.record(w); w.handle_requests([A((0,)), S(1)])
    quiet, moving = dc.make_delta("changed", [i["B8"], i["B64"]], [(i["B8"], 0)]), dc.make_delta("changed", [i["B8"], i["B32"]], [(i["B32"], 0)])
    for trust in (False, True):
        assert dc.assert_delta_equals_model(w, 1, 0, rec1, rec0, quiet, 300, trust_versions=trust)["n_matched"] == 0
        cols = int(w.kernel_info()["delta"].split("compared ")[1].split(" ")[0])
        assert cols == (0 if trust else 4), w.kernel_info()["delta"]                               # B8 {2} + B64 {2} words, or none of them
        assert dc.assert_delta_equals_model(w, 1, 0, rec1, rec0, moving, 300, trust_versions=trust)["n_matched"] == 300
        cols = int(w.kernel_info()["delta"].split("compared ")[1].split(" ")[0])
        assert cols == (2 if trust else 4), w.kernel_info()["delta"]                               # only B32's two words
    w.close()


def test_result_views_and_a_reused_buffer():
    sc = scene(129)
    i = sc.ids
    r = sc.w.delta(1, 0, [i["B16"], (i["B64"], 1)], changed=[i["B8"]])                             # a component id: all of its words; max_rows: the capacity
    want = dc.model_delta(sc.rec[1], sc.rec[0], dc.make_delta("changed", [i["B8"]], [(i["B16"], 0), (i["B16"], 1), (i["B16"], 2), (i["B64"], 1)]), sc.w.capacity)
    assert isinstance(r, bg.DeltaResult) and isinstance(r, bg.QueryResult) and r.kind == "changed"
    assert (r.n_matched, r.n_rows, r.len, r.len_new, r.len_old, r.n_beyond_old_len) == (want["n_matched"], want["n_rows"], 129 + NEAR, 129 + NEAR, 129, want["n_beyond_old_len"])
    assert [c.dtype for c in r.columns] == [torch.int16] * 3 + [torch.int64] and r.slots.dtype == torch.int32 and r.max_rows == sc.w.capacity
    slots, cols = r.numpy()
    assert np.array_equal(slots, want["slots"]) and all(np.array_equal(a, b) for a, b in zip(cols, want["columns"]))
    again = sc.w.delta(0, 1, kind="despawned", out=r.buffer, max_rows=4)                           # old-based: len is old's
    assert again.buffer is r.buffer and again.len == 129 + NEAR and again.n_beyond_old_len == 0
    with pytest.raises(ValueError): sc.w.delta(1, 0, [i["B64"]], changed=[i["B8"]], out=torch.empty(100, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError): sc.w.delta(1, 0, kind="moved")


# ---------------------------------------------------------------------------------------------------------------- sessions: every pair of held frames
def check_frame_pairs(w, descs, comps=None, extra=64):
    """Asks every desc of every ordered pair of frames the ring holds, of LIVE against the newest and back, and of each frame against a snapshot_copy of its
    predecessor; then loads the frames, newest first, and holds what was gathered against the model over the downloaded states.  Returns the frames."""
    frames = [f for f in range(w.frame + 1, w.frame - 40, -1) if w.has_snapshot(f)]
    assert len(frames) >= 2
    recs = {LIVE: qc.record(w, comps)}
    cap = recs[LIVE]["len"] + extra
    asks = [(a, b, None) for a in frames for b in frames if a != b] + [(LIVE, frames[0], None), (frames[0], LIVE, None)]
    asks += [(a, b, w.snapshot_copy(b)) for a, b in zip(frames, frames[1:])]
    got = {}
    for n_ask, (a, b, blk) in enumerate(asks):
        for k, desc in enumerate(descs): got[(n_ask, k)] = dc.device_delta(w, a, b if blk is None else blk, desc, cap)
    for f in frames:                                                                               # (a Load drops the frames behind it: newest first)
        w.handle_requests([L(f)])
        recs[f] = qc.record(w, comps)
    hit = {k: 0 for k in dc.KINDS}
    for n_ask, (a, b, blk) in enumerate(asks):
        for k, desc in enumerate(descs):
            want = dc.model_delta(recs[a], recs[b], desc, cap)
            dc.assert_answer_equals_model(w, got[(n_ask, k)], want, desc, cap, ctx=(a, b, blk is not None))
            hit[desc["kind"]] += want["n_matched"]
    return frames, hit


@pytest.mark.parametrize("forced", [False, True], ids=["default", "deferred_saves_lazy_live"])
def test_synctest_session_every_pair_of_ring_frames(forced):
    n = 3000
    w = bg.World(n + 4096, max_depth=8)
    ids = cm.build_particles(w, with_spawn=True)
    if forced: assert w._lib.ggrs_dbg_set_lazy_live(w._p, 3) == 0                                  # deferred Saves and the lazy live block on every eligible group
    vel, ttl = cm.synthetic_particles(n, ttl="despawn")
    cm.spawn_particles(w, ids, n, vel, ttl)
    drv, fn = cm.SyncTestDriver(w, 3), cm.frame_spawn_fn(rate=37)
    for t in range(30): drv.tick((cm.INPUT_SPAWN if t % 4 == 1 and t < 20 else 0,), spawn_fn=fn)
    if forced: assert cm.deferred_counts(w)[0] > 0, w.kernel_info()["deferred_saves"]
    T, V, Lc = ids[:3]
    descs = [dc.make_delta("changed", [T, V, Lc], [(T, 0), (T, 1), (V, 0), (Lc, 0)]), dc.make_delta("changed", [V], [], slots=True), dc.make_delta("added", [T], [(Lc, 0)]),
             dc.make_delta("removed", [Lc], [(T, 1)]), dc.make_delta("despawned", (), [(Lc, 0)], slots=False), dc.make_delta("despawned", ())]
    frames, hit = check_frame_pairs(w, descs)
    assert len(frames) >= 3 and hit["changed"] and hit["removed"] and hit["despawned"], hit       # ttl despawns happened between the held frames
    w.close()


def test_device_spawn_world_takes_len_from_the_header():
    import device_spawn_script as ds
    sc = ds.fans_across_empty_tiles()
    w = bg.World(sc.capacity, max_depth=sc.max_depth)
    ids = ds.build(w, sc)
    for step in sc.steps:
        if step[0] == "list": w.handle_requests(step[1])
    r = w.delta(2, 0, kind="added", changed=[ids[0]], max_rows=0)
    assert r.len_old == sc.n and r.len_new > r.len_old and r.len_new <= w.len                       # the device spawned: every frame has the len its Save wrote
    plan, plan2, mix, n16, n8 = ids
    descs = [dc.make_delta("changed", [plan, plan2, mix, n16, n8]), dc.make_delta("changed", [mix, n8], [(mix, 1), (n8, 0)]), dc.make_delta("added", [plan, plan2, mix], []),
             dc.make_delta("removed", [plan, plan2, mix, n16, n8], [(mix, 0)]), dc.make_delta("despawned", ())]
    frames, hit = check_frame_pairs(w, descs)
    assert len(frames) >= 3 and hit["changed"], hit
    w.close()


STRATEGY_SRC = ("__device__ void ggrs_store(const GgrsWords& t, GgrsWords& s) { s.u16(0) = (unsigned short)t.u32(0); }\n"
                "__device__ void ggrs_load(const GgrsWords& s, GgrsWords& t) { t.u32(0) = s.u16(0); }")


def test_strategy_component_is_compared_in_stored_form():
    w = bg.World(200, max_depth=4)
    Al = w.register_component("Alpha", 4, 1); Be = w.register_component("Beta", 4, 1)
    w.checksum_component(Al, [0]); w.checksum_component(Be, [0])
    w.register_component_strategy(Al, 2, 1, STRATEGY_SRC)
    w.add_system(bg.SYS_ADD_U32, comp=(Be,), word=(0,), iparam=(1,))
    w.set_depth(4)
    w.spawn(100, {Al: [np.arange(100, dtype=U32)], Be: [np.arange(100, dtype=U32) * 3]})
    for s in range(0, 100, 4): w.remove_component(Al, s)
    w.despawn(5)
    rec0 = qc.record(w)
    w.handle_requests([S(0)])
    a = w.download_word(Al, 0)
    a[10:20] += U32(0x10000)                                                                       # moves the live word and not the Stored one (its low 16 bits)
    a[30:40] += U32(1)                                                                             # moves both
    w.upload_word(Al, 0, 0, a)
    w.insert_component(Al, 8, np.array([8], dtype=U32))
    w.handle_requests([A((0,)), S(1)])
    rec1 = qc.record(w)
    stored = lambda rec: dict(rec, columns={k: (v & U32(0xFFFF) if k[0] == Al else v) for k, v in rec["columns"].items()})
    desc = dc.make_delta("changed", [Al], [(Be, 0)])
    for new, old in ((1, 0), (0, 1)):
        recs = {0: rec0, 1: rec1}
        want = dc.assert_delta_equals_model(w, new, old, stored(recs[new]), stored(recs[old]), desc, 100, ctx="Stored words")
        assert set(want["all_slots"].tolist()) == ({s for s in range(30, 40) if s % 4 and s != 5} | ({8} if new == 1 else set()))
        dc.assert_delta_equals_model(w, new, w.snapshot_copy(old), stored(recs[new]), stored(recs[old]), desc, 100, ctx="Stored words, a block")
    dc.assert_delta_equals_model(w, LIVE, LIVE, rec1, rec1, desc, 100, ctx="LIVE against LIVE: live words, nothing differs")
    for new, old in ((LIVE, 0), (0, LIVE), (LIVE, w.snapshot_copy(0))):
        with pytest.raises(bg.GgrsHipError) as e: dc.device_delta(w, new, old, desc, 100)
        assert e.value.code == bg.GGRS_E_INVALID and "not comparable" in str(e.value)
        for d in (dc.make_delta("added", [Al], [(Be, 0)]), dc.make_delta("changed", [Be], [(Be, 0)], with_=[Al])):      # masks are comparable; Beta is plain
            if new == LIVE: dc.assert_delta_equals_model(w, new, old, rec1, rec0, d, 100, ctx="masks only")
    with pytest.raises(bg.GgrsHipError) as e: dc.device_delta(w, 1, 0, dc.make_delta("changed", [Be], [(Al, 0)]), 100)
    assert e.value.code == bg.GGRS_E_INVALID and "Strategy" in str(e.value)                        # fetching it from a frame: refused as the query refuses it
    w.close()


# ---------------------------------------------------------------------------------------------------------------- the round trip
def test_round_trip_brings_a_world_from_one_frame_to_the_next():
    """Load(a), spawn what lies beyond a's len, INSERT the CHANGED rows of every component, REMOVE the REMOVED rows, DESPAWN the DESPAWNED rows: the live world is
    frame b.  A forward delta in a world without RollbackDespawned markers, every fresh entity alive in b (then the CHANGED rows of all components beyond a's len
    are len_b - len_a)."""
    n = 700
    w = bg.World(n + 400, max_depth=4)
    ids = cm.build_particles(w)
    T, V, Lc = ids[:3]
    w.set_depth(4)
    vel, ttl = cm.synthetic_particles(n, ttl="despawn")                                            # ttl 1 .. 300: the Advance below lets the shortest-lived die on the device
    cm.spawn_particles(w, ids, n, vel, ttl)
    for s in range(3, n, 17): w.remove_component(V, s)
    w.handle_requests([S(0)])
    for s in range(5, n, 9): w.despawn(s)
    alive = w.alive_mask()
    for s in range(6, n, 11):
        if alive[s]: w.remove_component(Lc, s)
    for s in range(3, n, 34):
        if alive[s]: w.insert_component(V, s, np.array([1.5, -2.5, 0.0], dtype=np.float32))
    for s in range(7, n, 23):
        if alive[s]: w.insert_component(T, s, np.arange(10, dtype=np.float32) + s)
    vel2, ttl2 = cm.synthetic_particles(90, ttl="throughput", seed=5)
    cm.spawn_particles(w, ids, 90, vel2, ttl2)
    w.handle_requests([A((0,)), S(1)])
    block_b, parts_b = w.snapshot_copy(1), w.checksum_parts(1)
    changed = {c: w.delta(1, 0, [c], kind="changed", changed=[c]) for c in ids[:3]}
    removed = {c: w.delta(1, 0, kind="removed", changed=[c]) for c in ids[:3]}
    despawned = w.delta(1, 0, kind="despawned")
    tail = w.delta(1, 0, kind="changed", changed=ids[:3], max_rows=0)
    assert tail.n_beyond_old_len == tail.len_new - tail.len_old == 90 and despawned.n_matched > 70 and all(r.n_matched for r in removed.values())
    w.handle_requests([L(0)])
    assert w.diff(LIVE, block_b).n_entities > 0
    w.spawn(tail.n_beyond_old_len, {})
    for c in ids[:3]:
        rep = w.scatter(changed[c], op="insert")
        assert rep.n_applied == changed[c].n_rows and rep.n_dead == 0 and rep.n_absent == 0
    for c in ids[:3]:
        rep = w.scatter(removed[c], op="remove", comps=[c])
        assert rep.n_applied == removed[c].n_rows
    rep = w.scatter(despawned, op="despawn")
    assert rep.n_applied == despawned.n_rows
    d = w.diff(LIVE, block_b)
    assert d.n_entities == 0 and d.n_alive == 0 and not d.n_presence and not d.n_value, d
    parts = w.checksum_parts(LIVE)
    assert parts.parts == parts_b.parts and parts.checksum == parts_b.checksum and (parts.len, parts.active) == (parts_b.len, parts_b.active)
    w.close()


# ---------------------------------------------------------------------------------------------------------------- errors
def test_refusals_and_no_snapshot():
    sc = scene(65)
    w, i = sc.w, sc.ids
    out = torch.empty(4096, dtype=torch.uint8, device="cuda")
    rep = _ffi.DeltaReport()

    def refused(desc, what, code=bg.GGRS_E_INVALID, new=1, old=0, out_ptr=out.data_ptr(), max_rows=4, report=True):
        rc = w._lib.ggrs_hip_delta_frames(w._p, new, old, C.byref(desc), out_ptr, max_rows, C.byref(rep) if report else None)
        msg = w._lib.ggrs_hip_last_error(w._p).decode()
        assert rc == code and msg and what in msg, (rc, msg)

    D = w.delta_desc
    d = D([(i["B8"], 0)], changed=[i["B8"]]); d.q.words[0].comp = 17
    refused(d, "component 17")
    refused(D([(i["B32"], 0)], changed=[i["B8"]], without=[i["B32"]]), "With")
    d = D(changed=[i["B8"]]); d.kind = 9
    refused(d, "unknown delta kind 9")
    d = D(changed=[i["B8"]]); d.flags = 4
    refused(d, "unknown delta flags")
    refused(D(changed=[33]), "does not have")
    refused(D(), "empty changed_mask")
    refused(D(kind="despawned", changed=[i["B8"]]), "DESPAWNED")
    refused(D(changed=[i["B8"]]), "without a report", report=False)
    refused(D([(i["B8"], 0)], changed=[i["B8"]]), "no output buffer", out_ptr=None)               # out_dev == NULL with max_rows > 0 ...
    assert w._lib.ggrs_hip_delta_frames(w._p, 1, 0, C.byref(D([(i["B8"], 0)], changed=[i["B32"]])), None, 0, C.byref(rep)) == 0 and rep.n_rows == 0      # ... and served with 0: a count
    assert rep.n_matched == dc.model_delta(sc.rec[1], sc.rec[0], dc.make_delta("changed", [i["B32"]], [(i["B8"], 0)]), 0)["n_matched"] > 0
    refused(D(changed=[i["B8"]]), "no snapshot", code=bg.GGRS_E_NO_SNAPSHOT, new=999)
    refused(D(changed=[i["B8"]]), "no snapshot", code=bg.GGRS_E_NO_SNAPSHOT, old=-7)
    rc = w._lib.ggrs_hip_delta_block(w._p, 1, None, C.byref(D(changed=[i["B8"]])), out.data_ptr(), 4, C.byref(rep))
    assert rc == bg.GGRS_E_INVALID and b"without a block" in w._lib.ggrs_hip_last_error(w._p)
    bad = sc.blocks[0].clone(); bad[:8] = torch.tensor(list((10 ** 9).to_bytes(8, "little")), dtype=torch.uint8)
    rc = w._lib.ggrs_hip_delta_block(w._p, 1, bad.data_ptr(), C.byref(D(changed=[i["B8"]])), out.data_ptr(), 4, C.byref(rep))
    assert rc == bg.GGRS_E_INVALID and b"not a block of this world" in w._lib.ggrs_hip_last_error(w._p)
    # outstanding batches: refused as the other synchronous calls are
    w.enqueue_requests([S(w.frame)])
    try:
        refused(D(changed=[i["B8"]]), "uncollected")
        rc = w._lib.ggrs_hip_delta_block(w._p, 1, sc.blocks[0].data_ptr(), C.byref(D(changed=[i["B8"]])), out.data_ptr(), 4, C.byref(rep))
        assert rc == bg.GGRS_E_INVALID and b"uncollected" in w._lib.ggrs_hip_last_error(w._p)
    finally:
        w.collect_checksums()
    _scenes.pop(65)                                                                                # (the Save above took a ring slot: the scene is no longer what its records say)
    w.close()
