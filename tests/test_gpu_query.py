"""The device query (ggrs_hip_query / ggrs_hip_query_block; World.query) against the numpy model of its semantics (tests/query_common.py).  Every comparison is
the device's whole output buffer -- pre-filled with 0xA5 -- against the model's rows laid out as the header says, bit for bit: the rows, the bytes beyond row
n_rows of every column and the padding between columns.  The model's inputs are the library's own download calls (alive, presence, words): the route a host
takes today."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import bevy_ggrs_amd as bg
import common as cm
import query_common as qc
from bevy_ggrs_amd import _ffi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [0, 1, 63, 64, 65, 8191, 8192, 8193, 8192 + 65, 3 * 8192 + 1]
U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
S, L, A = bg.SaveGameState, bg.LoadGameState, bg.AdvanceFrame


# ---------------------------------------------------------------------------------------------------------------- the edge worlds
class Edge:
    """A world of `n` entities with every word width.  Mark sits on every 7th slot, B16 is removed from every 11th; then every 13th slot is despawned, unit 1
    (slots 64..127) is wholly dead, unit 2 keeps only its lane 0 and unit 3 only its lane 63 -- as far as n reaches."""

    def __init__(self, n):
        self.n = n
        self.w = w = bg.World(n + 200, max_depth=4)
        self.ids = ids = qc.build_widths(w)
        w.set_depth(4)
        qc.spawn_widths(w, ids, n)
        for s in range(0, n, 7): w.insert_component(ids["Mark"], s, np.array([s ^ 0x5A5A5A], dtype=U32))
        for s in range(0, n, 11): w.remove_component(ids["B16"], s)
        dead = set(range(0, n, 13)) | set(range(64, 128)) | set(range(129, 192)) | set(range(192, 255))
        for s in sorted(x for x in dead if x < n): w.despawn(s)
        self.rec = qc.record(w)
        assert self.rec["len"] == n

    def check(self, desc, max_rows=None, ctx=""):
        return qc.assert_query_equals_model(self.w, bg.LIVE, self.rec, desc, self.n if max_rows is None else max_rows, ctx=(self.n, ctx))


_edges = {}


def edge(n):
    if n not in _edges: _edges[n] = Edge(n)
    return _edges[n]


def permuted_fetch(e):
    """Words of all four widths, several per component, not in column order."""
    i = e.ids
    return [(i["B64"], 1), (i["B8"], 0), (i["B32"], 1), (i["B16"], 2), (i["B8"], 1), (i["B64"], 0), (i["B16"], 0), (i["B32"], 0), (i["B16"], 1)]


@pytest.mark.parametrize("n", LENS)
def test_unit_and_tile_edges_all_widths(n):
    e = edge(n)
    alive = e.rec["alive"]
    if n > 255: assert not alive[64:128].any() and alive[128:192].tolist() == [True] + [False] * 63 and alive[192:256].tolist() == [False] * 63 + [True]
    want = e.check(qc.make_desc(permuted_fetch(e)), ctx="permuted")
    assert want["n_matched"] == int((alive & e.rec["present"][e.ids["B16"]]).sum())
    e.check(qc.make_desc(qc.all_words(e.w, e.ids, ("B8", "B16", "B32", "B64"))), ctx="in order")
    e.check(qc.make_desc(permuted_fetch(e), slots=False), ctx="no slots")
    want = e.check(qc.make_desc(), ctx="slots only, no filter")
    assert want["n_matched"] == e.w.active_count() == int(alive.sum())                             # an empty filter: every live entity


@pytest.mark.parametrize("n", [65, 8192 + 65])
def test_filters(n):
    e = edge(n)
    i, rec = e.ids, e.rec
    alive, mark, b16 = rec["alive"], rec["present"][i["Mark"]], rec["present"][i["B16"]]
    f32 = [(i["B32"], 0), (i["B64"], 1)]
    assert e.check(qc.make_desc(f32, with_=[i["Mark"]]), ctx="With")["n_matched"] == int((alive & mark).sum())
    assert e.check(qc.make_desc(f32, without=[i["Mark"]]), ctx="Without")["n_matched"] == int((alive & ~mark).sum())
    assert e.check(qc.make_desc(f32, with_=[i["Mark"]], without=[i["B16"]]), ctx="both")["n_matched"] == int((alive & mark & ~b16).sum())
    assert e.check(qc.make_desc([], with_=[i["Mark"]]), ctx="filter only, slots only")["n_matched"] == int((alive & mark).sum())
    assert e.check(qc.make_desc([], without=[i["B16"]], slots=False), ctx="nothing written")["n_matched"] == int((alive & ~b16).sum())
    assert e.check(qc.make_desc([(i["Mark"], 0)]), ctx="implicit With")["n_matched"] == int((alive & mark).sum())
    assert e.check(qc.make_desc([(i["Mark"], 0)], without=[i["B8"]]), ctx="empty")["n_matched"] == 0
    assert e.check(qc.make_desc(), ctx="empty filter")["n_matched"] == e.w.active_count()


@pytest.mark.parametrize("n", [65, 8192 + 65])
def test_truncation_leaves_everything_beyond_n_rows_untouched(n):
    e = edge(n)
    desc = qc.make_desc(permuted_fetch(e))
    full = qc.model_of(e.rec, desc, n)
    total = full["n_matched"]
    mid = next(k for k in range(total // 2, total) if full["slots"][k - 1] // 64 == full["slots"][k] // 64)      # the cut falls inside a 64-slot unit
    for cap in (0, 1, mid, total, total + 1):
        want = e.check(desc, cap, ctx=f"max_rows {cap}")                                          # (the 0xA5 bytes beyond the rows are part of the comparison)
        assert want["n_matched"] == total and want["n_rows"] == min(cap, total)
        assert want["slots"].tolist() == full["slots"][:cap].tolist()
        e.check(qc.make_desc([], with_=[e.ids["Mark"]]), cap, ctx=f"slots only, max_rows {cap}")


def test_launch_geometry_does_not_change_a_byte():
    e = edge(3 * 8192 + 1)
    desc = qc.make_desc(permuted_fetch(e), without=[e.ids["Mark"]])
    total = qc.model_of(e.rec, desc, e.n)["n_matched"]
    try:
        for cap in (e.n, total // 3):
            runs = []
            for grid in (0, 1, 2, 7, 0):                                                          # by size, capped to 1, 2 and 7 workgroups, by size again
                assert e.w._lib.ggrs_dbg_set_query_grid(e.w._p, grid) == 0
                runs.append(qc.device_query(e.w, bg.LIVE, desc, cap))
                e.check(desc, cap, ctx=f"grid {grid}")
            for r in runs[1:]: assert r[:2] == runs[0][:2] and np.array_equal(r[2], runs[0][2])
    finally:
        e.w._lib.ggrs_dbg_set_query_grid(e.w._p, 0)
    assert "query" in e.w.kernel_info()


def test_result_views_and_reused_buffer():
    e = edge(8193)
    i = e.ids
    r = e.w.query(bg.LIVE, [i["B16"], (i["B64"], 1)], without=[i["Mark"]])                         # a component id: all of its words; max_rows: the world's len
    want = qc.model_of(e.rec, qc.make_desc([(i["B16"], 0), (i["B16"], 1), (i["B16"], 2), (i["B64"], 1)], without=[i["Mark"]]), e.n)
    assert (r.n_matched, r.n_rows, r.len) == (want["n_matched"], want["n_rows"], e.n) and r.words == [(i["B16"], 0), (i["B16"], 1), (i["B16"], 2), (i["B64"], 1)]
    assert [c.dtype for c in r.columns] == [torch.int16] * 3 + [torch.int64] and r.slots.dtype == torch.int32 and all(c.is_cuda and c.numel() == r.n_rows for c in r.columns)
    assert r.columns[3].data_ptr() == r.buffer.data_ptr() + int(e.w.query_layout(e.w.query_desc([i["B16"], (i["B64"], 1)]), e.n).col_off[3])      # views, not copies
    slots, cols = r.numpy()
    assert np.array_equal(slots, want["slots"]) and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(cols, want["columns"]))
    again = e.w.query(bg.LIVE, [(i["B8"], 1)], out=r.buffer, max_rows=10)                           # a caller-owned buffer, reused
    assert again.buffer is r.buffer and again.n_rows == 10 and np.array_equal(again.numpy()[1][0], qc.model_of(e.rec, qc.make_desc([(i["B8"], 1)]), 10)["columns"][0])
    with pytest.raises(ValueError): e.w.query(bg.LIVE, [i["B64"]], out=torch.empty(100, dtype=torch.uint8, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- sides: ring frames, LIVE, blocks
def check_every_side(w, descs, comps=None):
    """Queries every frame the ring holds (as a frame and as snapshot_copy + query_block: the same bytes) and LIVE; then loads the frames, newest first, and holds
    what was gathered against the model over each frame's downloaded state.  Returns the frames."""
    frames = [f for f in range(w.frame + 1, w.frame - 40, -1) if w.has_snapshot(f)]
    assert len(frames) >= 2
    live_rec = qc.record(w, comps)
    for desc in descs: qc.assert_query_equals_model(w, bg.LIVE, live_rec, desc, live_rec["len"], ctx=("LIVE", desc))
    got = {}
    for f in frames:
        blk = w.snapshot_copy(f)
        for k, desc in enumerate(descs):
            cap = live_rec["len"] + 64
            got[(f, k)] = qc.device_query(w, f, desc, cap)
            via_block = qc.device_query(w, blk, desc, cap)
            assert via_block[:2] == got[(f, k)][:2] and np.array_equal(via_block[2], got[(f, k)][2]), (f, desc)
    for f in frames:                                                                               # (a Load drops the frames behind it: newest first)
        w.handle_requests([L(f)])
        rec = qc.record(w, comps)
        for k, desc in enumerate(descs):
            cap = live_rec["len"] + 64
            want = qc.model_of(rec, desc, cap)
            n_matched, n_rows, buf = got[(f, k)]
            assert (n_matched, n_rows) == (want["n_matched"], want["n_rows"]), (f, desc)
            assert np.array_equal(buf, qc.expected_buffer(want, qc.word_bytes_of(w, desc), cap, buf.size)), (f, desc)
    return frames


@pytest.mark.parametrize("forced", [False, True], ids=["default", "deferred_saves_lazy_live"])
def test_synctest_session_every_ring_frame_and_live(forced):
    n = 3000
    w = bg.World(n + 4096, max_depth=8)
    ids = cm.build_particles(w, with_spawn=True)
    if forced: assert w._lib.ggrs_dbg_set_lazy_live(w._p, 3) == 0                                  # deferred Saves and the lazy live block on every eligible group
    vel, ttl = cm.synthetic_particles(n, ttl="despawn")
    cm.spawn_particles(w, ids, n, vel, ttl)
    drv, fn = cm.SyncTestDriver(w, 3), cm.frame_spawn_fn(rate=37)
    for t in range(30): drv.tick((cm.INPUT_SPAWN if t % 4 == 1 and t < 20 else 0,), spawn_fn=fn)   # (a group that holds a host spawn is never deferred: the last ticks hold none)
    if forced: assert cm.deferred_counts(w)[0] > 0, w.kernel_info()["deferred_saves"]
    T, V, Lc = ids[:3]
    descs = [qc.make_desc([(T, 0), (T, 1), (T, 2), (V, 0), (V, 1), (Lc, 0)]), qc.make_desc([(Lc, 0)], slots=False), qc.make_desc()]
    assert int(w.alive_mask().sum()) < w.len                                                       # ttl despawns happened: dead slots below len
    frames = check_every_side(w, descs)
    assert len(frames) >= 3
    w.close()


def test_device_spawn_world_takes_len_from_the_header():
    import device_spawn_script as ds
    sc = ds.fans_across_empty_tiles()
    w = bg.World(sc.capacity, max_depth=sc.max_depth)
    ids = ds.build(w, sc)
    for step in sc.steps:
        if step[0] == "list": w.handle_requests(step[1])
    lens = [w.query(f, [], max_rows=0).len for f in (0, 1, 2)]
    assert lens[0] == sc.n and lens[0] <= lens[1] <= lens[2] <= w.len and lens[2] > lens[0]        # the device spawned: every frame has the len its Save wrote
    plan, plan2, mix, n16, n8 = ids
    descs = [qc.make_desc([(mix, 1), (n8, 0), (plan, 0), (n16, 0)]), qc.make_desc([(mix, 0)], without=[plan2]), qc.make_desc([], with_=[plan2])]
    frames = check_every_side(w, descs)
    assert len(frames) >= 3
    w.close()


def test_rollback_despawned_markers_and_a_non_rollback_component():
    import test_despawn_rollback as tdr
    n = 300
    w = bg.World(n + 50, max_depth=8)
    H, M = tdr.build(w, n)
    w.set_depth(8); w.set_confirmed(0)
    w.handle_requests([S(0)])
    for _ in range(3): w.handle_requests([A((0,))])                                                # health 1, 2, 3 die in unconfirmed frames: marked, not freed
    w.handle_requests([S(3)])
    health0 = 1 + (np.arange(n) % 5)
    assert np.array_equal(w.disabled_mask(n), health0 <= 3)
    rec = qc.record(w)
    health, both = qc.make_desc([(H, 0)]), qc.make_desc([(M, 1), (H, 0), (M, 0)])
    want = qc.assert_query_equals_model(w, bg.LIVE, rec, health, n, ctx="LIVE, marked entities")
    assert want["slots"].tolist() == np.flatnonzero(health0 > 3).tolist()                          # a marked entity is invisible
    want = qc.assert_query_equals_model(w, bg.LIVE, rec, both, n, ctx="LIVE, a non-rollback component")   # served on LIVE
    assert want["n_matched"] == int((health0 > 3).sum()) and want["columns"][2].tolist() == (np.flatnonzero(health0 > 3) + 1000).tolist()
    qc.assert_query_equals_model(w, bg.LIVE, rec, qc.make_desc([(H, 0)], with_=[M]), n, ctx="LIVE, filtering on it")
    f3, f0 = qc.device_query(w, 3, health, n), qc.device_query(w, 0, health, n)
    assert f3[0] == int((health0 > 3).sum()) and f0[0] == n                                        # absent from frame 3, all there in frame 0
    for desc, what in ((both, "fetch"), (qc.make_desc([(H, 0)], with_=[M]), "With"), (qc.make_desc([(H, 0)], without=[M]), "Without")):
        for state in (3, w.snapshot_copy(3)):
            with pytest.raises(bg.GgrsHipError) as e: qc.device_query(w, state, desc, n)           # live-only: refused on a frame and on a block
            assert e.value.code == bg.GGRS_E_INVALID and "not registered for rollback" in str(e.value), what
    for f, got in ((3, f3), (0, f0)):
        w.handle_requests([L(f)])
        r = qc.record(w)
        want = qc.model_of(r, health, n)
        assert got[:2] == (want["n_matched"], want["n_rows"]) and np.array_equal(got[2], qc.expected_buffer(want, [4], n, got[2].size)), f
    # after the rollback to frame 0 everybody is resurrected: present again on LIVE
    rec = qc.record(w)
    assert qc.assert_query_equals_model(w, bg.LIVE, rec, both, n, ctx="resurrected")["n_matched"] == n
    w.close()


STRATEGY_SRC = ("__device__ void ggrs_store(const GgrsWords& t, GgrsWords& s) { s.u16(0) = (unsigned short)t.u32(0); }\n"
                "__device__ void ggrs_load(const GgrsWords& s, GgrsWords& t) { t.u32(0) = s.u16(0); }")


def test_strategy_component():
    w = bg.World(200, max_depth=4)
    Al = w.register_component("Alpha", 4, 1); Be = w.register_component("Beta", 4, 1)
    w.checksum_component(Al, [0]); w.checksum_component(Be, [0])
    w.register_component_strategy(Al, 2, 1, STRATEGY_SRC)
    w.add_system(bg.SYS_ADD_U32, comp=(Be,), word=(0,), iparam=(1,))
    w.set_depth(4)
    w.spawn(100, {Al: [np.arange(100, dtype=U32)], Be: [np.arange(100, dtype=U32) * 3]})
    for s in range(0, 100, 4): w.remove_component(Al, s)
    w.despawn(5)
    w.handle_requests([S(0), A((0,)), S(1), A((0,))])
    rec = qc.record(w)
    qc.assert_query_equals_model(w, bg.LIVE, rec, qc.make_desc([(Al, 0), (Be, 0)]), 100, ctx="LIVE: live-form words are served")
    for state in (1, w.snapshot_copy(1)):
        with pytest.raises(bg.GgrsHipError) as e: qc.device_query(w, state, qc.make_desc([(Al, 0)]), 100)
        assert e.value.code == bg.GGRS_E_INVALID and "Strategy" in str(e.value)
    with_alpha, without_alpha = qc.make_desc([(Be, 0)], with_=[Al]), qc.make_desc([(Be, 0)], without=[Al])
    got = [qc.device_query(w, 1, d, 100) for d in (with_alpha, without_alpha)]                     # filtering on its presence in a frame is served
    w.handle_requests([L(1)])
    r = qc.record(w)
    for d, g in zip((with_alpha, without_alpha), got):
        want = qc.model_of(r, d, 100)
        assert g[:2] == (want["n_matched"], want["n_rows"]) and want["n_matched"] > 0 and np.array_equal(g[2], qc.expected_buffer(want, [4], 100, g[2].size))
    w.close()


# ---------------------------------------------------------------------------------------------------------------- errors
def test_refusals():
    e = edge(65)
    w, i = e.w, e.ids
    out = torch.empty(4096, dtype=torch.uint8, device="cuda")
    rep = _ffi.QueryReport()

    def refused(desc, what, code=bg.GGRS_E_INVALID, state=bg.LIVE, out_ptr=out.data_ptr(), max_rows=4):
        rc = w._lib.ggrs_hip_query(w._p, state, C.byref(desc), out_ptr, max_rows, C.byref(rep))
        msg = w._lib.ggrs_hip_last_error(w._p).decode()
        assert rc == code and msg and what in msg, (rc, msg)

    d = w.query_desc([(i["B8"], 0)]); d.words[0].comp = 17
    refused(d, "component 17")
    refused(w.query_desc([(i["B8"], 2)]), "word 2 of component B8")
    d = w.query_desc([]); d.n_words = _ffi.QUERY_MAX_WORDS + 1
    refused(d, "at most 32 words")
    refused(w.query_desc([], with_=[i["Mark"]], without=[i["Mark"]]), "With")
    refused(w.query_desc([(i["B32"], 0)], without=[i["B32"]]), "With")
    d = w.query_desc([]); d.flags = 2
    refused(d, "unknown query flags")
    refused(w.query_desc([(i["B8"], 0)]), "no output buffer", out_ptr=None)                         # out_dev == NULL with max_rows > 0 ...
    assert w._lib.ggrs_hip_query(w._p, bg.LIVE, C.byref(w.query_desc([(i["B8"], 0)])), None, 0, C.byref(rep)) == 0 and rep.n_matched == e.w.active_count() and rep.n_rows == 0   # ... and served with 0: a count
    refused(w.query_desc([(i["B8"], 0)]), "no snapshot", code=bg.GGRS_E_NO_SNAPSHOT, state=999)
    rc = w._lib.ggrs_hip_query_block(w._p, None, C.byref(w.query_desc([])), out.data_ptr(), 4, C.byref(rep))
    assert rc == bg.GGRS_E_INVALID and b"without a block" in w._lib.ggrs_hip_last_error(w._p)
    # outstanding batches: refused as the other synchronous calls are
    w.set_frame(0); w.enqueue_requests([S(0)])
    try:
        refused(w.query_desc([(i["B8"], 0)]), "uncollected")
        rc = w._lib.ggrs_hip_query_block(w._p, out.data_ptr(), C.byref(w.query_desc([])), out.data_ptr(), 4, C.byref(rep))
        assert rc == bg.GGRS_E_INVALID and b"uncollected" in w._lib.ggrs_hip_last_error(w._p)
    finally:
        w.collect_checksums()
    e.check(qc.make_desc([(i["B8"], 0)]), ctx="after the refusals")
    qc.assert_query_equals_model(w, 0, e.rec, qc.make_desc(permuted_fetch(e)), 65, ctx="the frame just saved")
    # (a Strategy fetch and a non-rollback component against a frame or a block: test_strategy_component, test_rollback_despawned_markers_and_a_non_rollback_component;
    #  GGRS_QUERY_SLOTS beyond 2^32 slots: no such world can be created, tests/test_query_model.py)


# ---------------------------------------------------------------------------------------------------------------- the C++ mirror
def test_cpp_mirror_query():
    src, out_dir = os.path.join(ROOT, "tests", "cpp", "query_host.cpp"), os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "query_host")
    deps = [src, os.path.join(ROOT, "include", "bevy_ggrs_hip.hpp"), os.path.join(ROOT, "include", "ggrs_hip.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps)):
        d = os.path.join(ROOT, "bevy_ggrs_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT}/include", "-isystem", "/opt/rocm/include", src, "-o", exe,
                               f"-L{d}", "-lggrs_hip", f"-Wl,-rpath,{d}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "ok query_live_and_frame" in out, out


# ---------------------------------------------------------------------------------------------------------------- fuzz
_fuzz_hit = {}


def _apply(w, comps, op):
    if op[0] == "spawn":
        _, count, which, salt = op
        s = np.arange(w.len, w.len + count)
        w.spawn(count, {c: [qc.fuzz_value(s, c, k, salt, comps[c][1]) for k in range(comps[c][2])] for c in sorted(which)})
    elif op[0] == "despawn": w.despawn(op[1])
    elif op[0] == "remove": w.remove_component(op[1], op[2])
    elif op[0] == "insert":
        _, c, s, salt = op
        w.insert_component(c, s, np.concatenate([qc.fuzz_value(s, c, k, salt, comps[c][1]) for k in range(comps[c][2])]))


def _assert_rec_is_shadow(rec, sh, ctx):
    """The downloaded state against the plan's numpy shadow, where it is state: alive bits, presence of the living, words of the present."""
    assert rec["len"] == sh["len"] and np.array_equal(rec["alive"], sh["alive"]), ctx
    for c, p in sh["present"].items():
        assert np.array_equal(rec["present"][c] & rec["alive"], p & sh["alive"]), (ctx, c)
    for key, col in sh["columns"].items():
        on = sh["alive"] & sh["present"][key[0]]
        assert np.array_equal(rec["columns"][key][on], col[on]), (ctx, key)


@pytest.mark.parametrize("seed", range(qc.FUZZ_SEEDS))
def test_fuzz(seed):
    comps, before, between, descs = qc.fuzz_plan(seed)
    _, sh0, sh_live, _ = qc.fuzz_shadow_states(seed)
    w = bg.World(qc.FUZZ_CAPACITY, max_depth=4)
    for name, wb, nw in comps: w.checksum_component(w.register_component(name, wb, nw), list(range(nw)))
    w.add_system(bg.SYS_ADD_U32, comp=(0,), word=(0,), iparam=(1,))
    w.set_depth(4)
    for op in before: _apply(w, comps, op)
    rec0 = qc.record(w)
    _assert_rec_is_shadow(rec0, sh0, "Save(0)")
    w.handle_requests([S(0)])
    for op in between: _apply(w, comps, op)
    w.handle_requests([A((0,)), S(1), A((0,))])
    live = qc.record(w)
    _assert_rec_is_shadow(live, sh_live, "LIVE")
    hit = set()
    for state, rec in ((0, rec0), (bg.LIVE, live)):
        for desc, cap in descs:
            cap = rec["len"] if cap is None else cap
            r = qc.assert_query_equals_model(w, state, rec, desc, cap, ctx=(seed, state, desc, cap))
            hit |= {f"width{comps[c][1]}" for c, _ in desc["fetch"]}
            if desc["with"]: hit.add("with")
            if desc["without"]: hit.add("without")
            if r["n_rows"] < r["n_matched"]: hit.add("truncated")
            if r["n_matched"] == 0: hit.add("empty")
            if r["n_matched"] > 64: hit.add("many_units")
    assert hit == qc.fuzz_coverage(seed)                                                           # the device run exercised what the CPU said this seed would
    _fuzz_hit[seed] = hit
    w.close()


def test_fuzz_coverage_floors():
    """Every width, With and Without, a truncated and an empty result, a result of more than one unit: each is hit by some seed.  The floors are computed here on
    the CPU, with the model over the plan's numpy shadow, from the same seeds; the seeds that ran on the device in this process hit exactly what was computed."""
    cover = {seed: qc.fuzz_coverage(seed) for seed in range(qc.FUZZ_SEEDS)}
    for what in qc.FUZZ_FLOORS:
        assert sum(what in c for c in cover.values()) >= 2, what
    for seed, hit in _fuzz_hit.items(): assert hit == cover[seed], seed
