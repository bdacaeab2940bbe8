"""The device's checksum parts (ggrs_hip_checksum_parts / ggrs_hip_checksum_parts_block) against the numpy model of their semantics
(tests/checksum_parts_common.py) and against the Checksum every SaveGameState returned, at the wave-unit (64) and layout-tile (8192) edges.  One world per size runs
ONE script of Saves with host edits between them; every Save's arrays are recorded through the download calls, every frame stays in the ring."""
import ctypes as C

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import checksum_parts_common as cp
import common as cm
import device_spawn_script as dss
import state_diff_common as sd
from bevy_ggrs_amd import _ffi
from bevy_ggrs_amd.session import MismatchedChecksum, SyncTestSession
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 8191, 8192, 8193, 2 * 8192 + 5]
U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
LABELS = ["s0", "same", "advanced", "one_value", "uploads", "structure", "entities", "resource", "planted_a", "planted_b"]
SEA_ONE_0 = onp.SeaHasher().write_u64(0).finish()


class Scenario:
    def __init__(self, n, vtags=False):
        self.n = n
        self.w = w = bg.World(n + 70, max_depth=12)
        self.s = s = sd.build_schema(w)
        self.specs = cp.schema_specs(s)
        if vtags: assert w._lib.ggrs_dbg_set_value_tags(w._p, 1) == 0
        w.set_depth(12)
        sd.spawn_schema(w, s, n)
        if vtags: assert w.kernel_info()["value_tags"].startswith("on"), w.kernel_info()["value_tags"]
        self.frames, self.recs, self.saved = {}, {}, {}
        ids, at = s.ids, lambda k: k % n
        self._f = 0
        self.snap("s0")
        self.snap("same")                                                      # two Saves with nothing between them
        w.handle_requests([sd.adv(1)]); self.snap("advanced")                  # one Advance apart: Pos.x, Big and the Clock moved
        w.upload_word(ids["Big"], 0, at(64), np.array([(1 << 63) | 5], dtype=U64)); self.snap("one_value")
        # upload_word on every word width
        w.upload_word(ids["Flag"], 0, at(2), np.array([200], dtype=U8)); w.upload_word(ids["Tag"], 0, at(8), np.array([65000], dtype=U16))
        w.upload_word(ids["Pos"], 1, at(63), np.array([0x80000000], dtype=U32)); w.upload_word(ids["Big"], 0, at(65), np.array([77], dtype=U64))
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
        w.upload_word(ids["Pos"], 0, p, np.array([2222], dtype=U32)); w.upload_word(ids["Big"], 0, q, np.array([3333], dtype=U64))   # under a dead slot, under an absent component
        w.upload_word(ids["Quiet"], 0, at(4), np.array([5555], dtype=U32))     # a word no checksum names
        w.upload_word(ids["Side"], 0, 0, np.array([777], dtype=U32))           # a non-rollback component
        self.snap("planted_b")

    def snap(self, label):
        self.w.set_frame(self._f)
        self.recs[label] = sd.record(self.w, self.s)
        self.saved[label] = self.w.save()
        self.frames[label] = self._f
        self._f += 1

    def model(self, label): return cp.model_parts(self.recs[label], self.specs)

    def device(self, label): return self.w.checksum_parts(self.frames[label])


_cache = {}


def scenario(n, vtags=False):
    if (n, vtags) not in _cache: _cache[(n, vtags)] = Scenario(n, vtags)
    return _cache[(n, vtags)]


@pytest.mark.parametrize("n", SIZES)
def test_every_save_matches_the_model_and_the_checksum_it_returned(n):
    sc = scenario(n)
    assert all(sc.w.has_snapshot(f) for f in sc.frames.values())
    for label in LABELS:
        got, want = sc.device(label), sc.model(label)
        assert cp.as_model(got) == want, (label, str(got))                     # the parts in their order, n_hashed, len, active and the XOR
        assert list(got.parts) == ["Flag", "Tag", "Pos", "Big", "Entity", "Clock"]
        assert got.checksum == sc.saved[label], label                          # the defining property: what this frame's SaveGameState returned
    assert sc.model("s0")["len"] == n and sc.model("entities")["len"] == n + 3


@pytest.mark.parametrize("n", SIZES)
def test_what_moves_which_part(n):
    sc = scenario(n)
    d = lambda a, b: sc.device(a).differing(sc.device(b))
    m = lambda a, b: [k for k in sc.model(a)["parts"] if sc.model(a)["parts"][k] != sc.model(b)["parts"][k]]
    assert d("s0", "same") == []
    assert d("same", "advanced") == ["Pos", "Big", "Clock"]                    # bump moves Pos.x and Big of every entity, tick the Clock
    assert d("advanced", "one_value") == ["Big"]                               # one word of one entity: exactly that component's part
    assert d("one_value", "uploads") == m("one_value", "uploads") and "Entity" not in d("one_value", "uploads") and "Clock" not in d("one_value", "uploads")
    moved = d("structure", "entities")                                         # a despawn and a spawn: the entity part and the components the entities hold
    assert moved == m("structure", "entities") and {"Entity", "Flag", "Pos", "Big"} <= set(moved) and "Clock" not in moved
    assert d("entities", "resource") == ["Clock"]                              # a resource write moves only the resource's part
    a, b = sc.device("planted_a"), sc.device("planted_b")                      # planted bytes are not state
    assert a.differing(b) == [] and a == b


@pytest.mark.parametrize("n", SIZES)
def test_the_live_world_right_after_a_save_and_a_snapshot_copy(n):
    sc = scenario(n)
    last = LABELS[-1]
    assert sc.w.checksum_parts(bg.LIVE) == sc.device(last)
    for label in ("advanced", "entities"):
        blk = sc.w.snapshot_copy(sc.frames[label])
        assert sc.w.checksum_parts(blk) == sc.device(label), label


@pytest.mark.parametrize("n", [65, 2 * 8192 + 5])
def test_the_grid_does_not_change_the_report(n):
    sc = scenario(n)
    try:
        for label in LABELS:
            runs = []
            for grid in (1, 2, 3, 0):                                          # one workgroup, two, three, and by size
                assert _ffi.lib.ggrs_dbg_set_parts_grid(sc.w._p, grid) == 0
                runs.append(sc.device(label))
            assert all(r == runs[0] for r in runs) and cp.as_model(runs[0]) == sc.model(label), label
    finally:
        _ffi.lib.ggrs_dbg_set_parts_grid(sc.w._p, 0)


@pytest.mark.parametrize("n", [65, 8193])
def test_value_tags_forced_on_give_the_same_parts(n):
    on, off = scenario(n, vtags=True), scenario(n)
    for label in LABELS:
        got = on.device(label)
        assert got == off.device(label) and cp.as_model(got) == on.model(label) and got.checksum == on.saved[label], label


def test_frames_made_by_request_lists_with_deferred_saves_and_the_lazy_live_block():
    """A steady SyncTest session with the lazy live block and deferred Saves forced on: the later Saves of a tick are owed to the ring, its last AdvanceFrame to the
    live block.  The parts of every frame the ring holds fold to the checksum the list returned for it; the call brings the slots up to date first."""
    n, cd = 8193, 3
    w = bg.World(n, max_depth=8)
    s = sd.build_schema(w, with_side=False)
    assert w._lib.ggrs_dbg_set_lazy_live(w._p, 3) == 0
    sd.spawn_schema(w, s, n)
    drv = cm.SyncTestDriver(w, cd)
    for _ in range(9): drv.tick((1,))
    deferred, materialised = cm.deferred_counts(w)
    assert deferred > 0, w.kernel_info()["deferred_saves"]
    returned = dict(drv.all_checksums)                                         # frame -> the checksum of its last Save
    held = [f for f in returned if w.has_snapshot(f)]
    assert len(held) >= cd + 1
    for f in held:
        p = w.checksum_parts(f)
        assert p.checksum == returned[f] and p.len == n and p.counts["Pos"] == n, f
    assert cm.deferred_counts(w)[1] > materialised
    newest = max(held)
    assert w.checksum_parts(newest - 1).differing(w.checksum_parts(newest)) == ["Pos", "Big", "Clock"]
    live = w.checksum_parts(bg.LIVE)                                           # one AdvanceFrame with input 1 beyond the newest frame
    assert live.differing(w.checksum_parts(newest)) == ["Pos", "Big", "Clock"] and live.parts["Entity"] == w.checksum_parts(newest).parts["Entity"]
    w.close()


def test_a_world_without_checksummed_components_has_the_entity_part_alone():
    w = bg.World(200, max_depth=4)
    X = w.register_component("X", 4, 1)
    w.add_system(bg.SYS_ADD_U32, comp=(X,), word=(0,), iparam=(1,))
    w.set_depth(4)
    w.spawn(130, {X: [np.arange(130, dtype=U32)]}); w.despawn(5)
    (cs,) = w.handle_requests([bg.SaveGameState(0)])
    p = w.checksum_parts(0)
    assert p.parts == {"Entity": onp.entity_checksum(129, 130)} and p.checksum == cs and (p.len, p.active) == (130, 129)
    w.close()


def test_a_checksummed_component_nobody_holds_is_sea_one_of_zero():
    w = bg.World(200, max_depth=4)
    X = w.register_component("X", 4, 1); N = w.register_component("Nobody", 8, 2)
    w.checksum_component(X, [0]); w.checksum_component(N, [1, 0])
    w.add_system(bg.SYS_ADD_U32, comp=(X,), word=(0,), iparam=(1,))
    w.set_depth(4)
    w.spawn(70, {X: [np.arange(70, dtype=U32)]})
    (cs,) = w.handle_requests([bg.SaveGameState(0)])
    p = w.checksum_parts(0)
    assert p.parts["Nobody"] == SEA_ONE_0 != 0 and p.counts == {"X": 70, "Nobody": 0, "Entity": 70} and p.checksum == cs
    w.insert_component(N, 3, np.array([1, 2], dtype=U64)); w.despawn(3)        # its only holder is dead: still nobody
    w.set_frame(1)
    assert w.save() == w.checksum_parts(1).checksum and w.checksum_parts(1).parts["Nobody"] == SEA_ONE_0
    w.close()


HASHER = ("__device__ ggrs_u64 ggrs_hash(const GgrsComponent& c) {\n"
          "    GgrsHasher h; h.write_u32(c.u32(0) ^ (c.u32(1) * 3u)); h.write_u8(c.u8(3) & 1); h.write_u64((ggrs_u64)c.u16(2) << 7);\n"
          "    return h.finish() ^ 0x55ull ^ (c.slot * 3ull);\n}\n")


def np_hasher(words, slots):
    """HASHER restated in numpy."""
    with np.errstate(over="ignore"):
        a = words[0] ^ (words[1] * U32(3))
    inner = onp.np_inner_hash_fields([(a, 4), (words[3] & U32(1), 1), ((words[2].astype(U64) & U64(0xFFFF)) << U64(7), 8)])
    with np.errstate(over="ignore"):
        return inner ^ U64(0x55) ^ (slots * U64(3))


@pytest.mark.parametrize("n", [65, 8193])
def test_a_world_with_a_user_written_hasher(n):
    w = bg.World(n + 8, max_depth=8)
    X = w.register_component("X", 4, 4); Y = w.register_component("Y", 2, 2)
    w.add_system(bg.SYS_ADD_U32, comp=(X,), word=(1,), iparam=(5,))
    w.checksum_component_custom(X, HASHER); w.checksum_component(Y, [1, 0])
    w.set_depth(8)
    r = np.random.default_rng(3)
    i = np.arange(n)
    w.spawn(n, {X: [r.integers(0, 2 ** 32, n, dtype=np.uint64).astype(U32) for _ in range(4)], Y: [(i * 5 % 65536).astype(U16), (i * 9 % 65536).astype(U16)]})
    for k in range(0, n, 4): w.remove_component(X, k)
    specs = cp.Specs([("X", X, np_hasher), ("Y", Y, [(1, 2), (0, 2)])])
    edits = [lambda: None, lambda: w.despawn(n - 1), lambda: w.upload_word(X, 3, 1, np.array([0xFFFFFFFF], dtype=U32)), lambda: w.handle_requests([bg.AdvanceFrame((0,))])]
    calls = 0
    for f, edit in enumerate(edits):
        edit()
        w.set_frame(f)
        rec = cp.record_words(w, [(X, 4), (Y, 2)])
        cs = w.save()
        p = w.checksum_parts(f); calls += 1
        assert cp.as_model(p) == cp.model_parts(rec, specs), f
        assert p.checksum == cs and p.counts["X"] == int((rec["alive"] & rec["present"][X]).sum()), f
    assert w.checksum_parts(bg.LIVE) == w.checksum_parts(len(edits) - 1); calls += 2
    assert w.checksum_parts(w.snapshot_copy(1)) == w.checksum_parts(1); calls += 2
    info = w.kernel_info()["checksum_parts"]                                   # every call after the first reused the module the first one made
    assert info.startswith(f"{calls} calls") and "ggrs_jit_parts" in info and "1 built or loaded by this world" in info, info
    w.close()


def test_a_world_that_defers_despawns_with_a_marker_pending():
    n = 300
    w = bg.World(n, max_depth=8)
    H = w.register_component("Health", 4, 1); M = w.register_component("Mesh", 4, 2, rollback=False)
    w.checksum_component(H, [0])
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, bg.DESPAWN_ROLLBACK))
    w.spawn(n, {H: [(1 + (np.arange(n) % 5)).astype(U32)], M: [np.arange(n, dtype=U32), np.arange(n, dtype=U32)]})
    w.set_depth(8); w.set_confirmed(0)
    reqs = [q for f in range(4) for q in (bg.SaveGameState(f), bg.AdvanceFrame((0,)))] + [bg.SaveGameState(4)]
    cs = w.handle_requests(reqs)
    assert w.disabled_mask(n).any()                                            # frames 1 .. 4 were saved while RollbackDespawned markers were pending
    for f in range(5):
        p = w.checksum_parts(f)
        assert p.checksum == cs[f] and p.len == n, f
    assert [w.checksum_parts(f).active for f in range(5)] == [n - (n // 5) * f for f in range(5)]
    assert w.checksum_parts(bg.LIVE) == w.checksum_parts(4)
    cs2 = w.handle_requests([bg.LoadGameState(1), bg.AdvanceFrame((0,)), bg.SaveGameState(2)])       # the markers of frames 2 .. 4 are undone by the Load
    assert w.checksum_parts(2).checksum == cs2[0] == cs[2]
    w.close()


@pytest.mark.parametrize("form", ["1", "2"], ids=["resident", "streamed"])
@pytest.mark.parametrize("n", [1, 65])
def test_a_world_that_spawns_on_the_device(n, form, monkeypatch):
    monkeypatch.setenv("GGRS_TICK_JIT", form)
    sc = dss.len_edge(n, 2)
    w = bg.World(sc.capacity, max_depth=sc.max_depth)
    dss.build(w, sc)
    returned = {}
    for step in sc.steps:
        if step[0] != "list": continue
        saves = [q.frame for q in step[1] if isinstance(q, bg.SaveGameState)]
        returned.update(zip(saves, w.handle_requests(step[1])))
    assert sorted(returned) == [0, 1, 2] and all(w.has_snapshot(f) for f in returned)
    lens = {f: w.checksum_parts(f).len for f in returned}
    for f in returned: assert w.checksum_parts(f).checksum == returned[f], (f, lens)
    assert lens[0] == n and lens[1] > n and lens[2] > lens[1]                  # RollbackOrdered::len of a frame: read from the slot's header
    assert w.checksum_parts(bg.LIVE) == w.checksum_parts(2)                    # the last list ends in Save(2)
    w.close()


def test_refusals():
    sc = scenario(64)
    w = sc.w
    with pytest.raises(bg.GgrsHipError) as e: w.checksum_parts(999)
    assert e.value.code == bg.GGRS_E_NO_SNAPSHOT and "999" in str(e.value)
    rep, arr = _ffi.PartsReport(), (_ffi.ChecksumPart * _ffi.MAX_PARTS)()
    assert w._lib.ggrs_hip_checksum_parts(w._p, sc.frames["s0"], C.byref(rep), arr, 5) == bg.GGRS_E_INVALID      # the world has 6 parts
    assert b"max_parts 5" in _ffi.lib.ggrs_hip_last_error(w._p) and b"6 checksum parts" in _ffi.lib.ggrs_hip_last_error(w._p)
    assert w._lib.ggrs_hip_checksum_parts(w._p, sc.frames["s0"], C.byref(rep), arr, 6) == 0 and rep.n_parts == 6 and rep.checksum_hi == 0
    assert [arr[i].kind for i in range(6)] == [0, 0, 0, 0, 1, 2] and arr[4].id == 0 and arr[5].id == sc.s.clock and arr[4].n_hashed == rep.active
    # outstanding batches: refused as the other synchronous calls are
    w.set_frame(sc._f); w.enqueue_requests([bg.SaveGameState(sc._f)])
    try:
        with pytest.raises(bg.GgrsHipError) as e: w.checksum_parts(sc.frames["s0"])
        assert e.value.code == bg.GGRS_E_INVALID and "uncollected" in str(e.value)
        with pytest.raises(bg.GgrsHipError) as e: w.checksum_parts(bg.LIVE)
        assert e.value.code == bg.GGRS_E_INVALID
    finally:
        (cs,) = w.collect_checksums()
    assert w.checksum_parts(sc._f).checksum == cs
    # a world with a checksummed component under a Strategy: a ring frame and a block are refused, the live world is served
    g = bg.World(200, max_depth=4)
    A = g.register_component("Alpha", 4, 1); B = g.register_component("Beta", 4, 1)
    g.checksum_component(A, [0]); g.checksum_component(B, [0])
    g.register_component_strategy(A, 2, 1, "__device__ void ggrs_store(const GgrsWords& t, GgrsWords& s) { s.u16(0) = (unsigned short)t.u32(0); }\n"
                                           "__device__ void ggrs_load(const GgrsWords& s, GgrsWords& t) { t.u32(0) = s.u16(0); }")
    g.add_system(bg.SYS_ADD_U32, comp=(B,), word=(0,), iparam=(1,))
    g.set_depth(4)
    g.spawn(100, {A: [np.arange(100, dtype=U32)], B: [np.arange(100, dtype=U32)]})
    cs = g.handle_requests([bg.SaveGameState(0), bg.AdvanceFrame((0,)), bg.SaveGameState(1)])
    with pytest.raises(bg.GgrsHipError) as e: g.checksum_parts(1)
    assert e.value.code == bg.GGRS_E_INVALID and "Strategy" in str(e.value) and "Alpha" in str(e.value)
    with pytest.raises(bg.GgrsHipError) as e: g.checksum_parts(g.snapshot_copy(1))
    assert e.value.code == bg.GGRS_E_INVALID and "Strategy" in str(e.value)
    live = g.checksum_parts(bg.LIVE)                                           # the live world is frame 1 as it was saved
    assert live.checksum == cs[1] and list(live.parts) == ["Alpha", "Beta", "Entity"] and live.counts["Alpha"] == 100
    g.close()


# ---- SyncTestSession(localise=True): which ChecksumPart (tests/test_gpu_synctest_localise.py makes the desync the same way)
N, CD, SLOT, PLANTED = 200, 2, 137, 0xABCD


def _run(localise, strategy=False):
    w = bg.World(N, max_depth=8)
    if strategy:
        A = w.register_component("Alpha", 4, 1); B = w.register_component("Beta", 4, 1)
        w.checksum_component(A, [0]); w.checksum_component(B, [0])
        w.register_component_strategy(A, 2, 1, "__device__ void ggrs_store(const GgrsWords& t, GgrsWords& s) { s.u16(0) = (unsigned short)t.u32(0); }\n"
                                               "__device__ void ggrs_load(const GgrsWords& s, GgrsWords& t) { t.u32(0) = s.u16(0); }")
        w.add_system(bg.SYS_ADD_U32, comp=(B,), word=(0,), iparam=(1,))
        w.spawn(N, {A: [np.arange(N, dtype=U32)], B: [np.arange(N, dtype=U32)]})
        edit = lambda: w.upload_word(B, 0, SLOT, np.array([PLANTED], dtype=U32))
    else:
        s = sd.build_schema(w)
        sd.spawn_schema(w, s, N)
        edit = lambda: w.upload_word(s.ids["Pos"], 1, SLOT, np.array([PLANTED], dtype=U32))
    w.set_depth(8); w.set_synctest_check_distance(CD)
    sess = SyncTestSession(1, CD, 8, localise=localise)
    calls, inner = [], w.checksum_parts

    def counted(state):
        calls.append("block" if hasattr(state, "data_ptr") else state)
        return inner(state)
    w.checksum_parts = counted

    def tick(edit=None):
        sess.add_local_input(0, 1)
        reqs = sess.advance_frame()
        cut = max(i for i, r in enumerate(reqs) if isinstance(r, bg.SaveGameState)) if edit else len(reqs)
        cs = w.handle_requests(reqs[:cut])
        if edit:
            edit()
            cs += w.handle_requests(reqs[cut:])
        sess.record_checksums(cs, world=w)

    for _ in range(6): tick()
    F = sess.current_frame
    tick(edit=edit)
    tick()                                                                     # re-saves F without the edit
    with pytest.raises(MismatchedChecksum) as e: tick()
    return w, F, e.value, calls


def test_localise_names_the_part():
    w, F, exc, calls = _run(True)
    assert exc.mismatched_frames == [F] and list(exc.parts) == [F] and list(exc.diffs) == [F]
    kept, resim = exc.parts[F]
    assert kept.differing(resim) == ["Pos"] and kept.counts == resim.counts and kept.len == resim.len == N
    assert kept.checksum != resim.checksum and kept.checksum ^ resim.checksum == kept.parts["Pos"] ^ resim.parts["Pos"]
    assert calls == ["block", F]                                               # the kept copy through the block call, the ring's frame through the frame call
    w.close()


def test_without_localise_no_parts_call_is_made():
    w, F, exc, calls = _run(False)
    assert exc.mismatched_frames == [F] and not hasattr(exc, "parts") and not hasattr(exc, "diffs") and calls == []
    assert "checksum_parts" not in w.kernel_info()
    w.close()


def test_localise_in_a_world_whose_parts_are_refused_keeps_the_diffs():
    w, F, exc, calls = _run(True, strategy=True)
    assert exc.mismatched_frames == [F] and not hasattr(exc, "parts") and calls == ["block"]
    assert exc.diffs[F].n_entities == 1 and exc.diffs[F].entries[0].slot == SLOT and exc.diffs[F].entries[0].first_name == "Beta"
    w.close()
