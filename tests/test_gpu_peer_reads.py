"""Cross-entity reads for user-written systems (ggrs_hip_add_custom_system_peers): a system follows a link -- a stable slot in an 8-byte word -- with
e.peer(slot) and reads the other entity's peer-bound words as they were at the START of the frame.  Everything goes through the C ABI and is bit-exact:
the Checksum(u128) of every SaveGameState and the final state equal the CPU oracle's, whose callbacks read the oracle's own columns (peer_reads_common.py).

The reference lets any system take a second Query (tests/hierarchy.rs: a child follows its ChildOf parent); here the view of the other entities is filled by
one small launch ahead of every request group that holds an AdvanceWorld, and such a world's groups hold one AdvanceWorld each."""
import ctypes as C
import os

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
from bevy_ggrs_amd import _ffi
from oracle.binding import FLAT, OracleWorld
from peer_reads_common import build_follow, children, follow_links, spawn_follow, spawn_patch

pytestmark = pytest.mark.gpu


def _compare(a, b, ctx):
    assert len(a[0]) == len(b[0]) > 0, (len(a[0]), len(b[0]))
    for (fa, ca), (fb, cb) in zip(a[0], b[0]):
        assert fa == fb and ca == cb, f"{ctx}: frame {fa}: gpu {ca:#x} oracle {cb:#x}"
    cm.assert_states_equal(a[1], b[1], ctx)


def _pair(cap, depth=8):
    return bg.World(cap, max_depth=depth), OracleWorld(cap, depth, FLAT)


def _synctest(w, n, cd, ticks, *, n_bare=0, with_spawn=False, links=None, check=None):
    ids = build_follow(w, with_spawn=with_spawn)
    spawn_follow(w, ids, n, n_bare=n_bare, links=links)
    drv = cm.SyncTestDriver(w, cd)
    patch = spawn_patch(n) if with_spawn else None
    for t in range(ticks):
        drv.tick((t & 3,), patch=patch)
    if check: check(w)
    return drv.all_checksums, cm.snapshot_state(w, ids)


def _is_peer_world(w):
    info = w.kernel_info()
    assert info["request_group_kernel"].startswith("ggrs_jit_tick"), info
    assert info["group_caps"].endswith("/ 1 steps") and info["peer_view"].startswith("2 linear columns"), info
    assert info["lazy_live_block"].startswith("off") and info["deferred_saves"].startswith("off"), info


def test_follow_600_slots_synctest_against_the_oracle():
    """Links (i * 389 + 17) % n cross 64-slot units and 256-slot workgroups; a tenth point at n + 5 (out of range), others at entities without Pos and at
    slots whose countdown runs out mid-session.  SyncTest check distance 3, 12 ticks."""
    n = 600
    g, o = _pair(n + 64)
    a = _synctest(g, n, 3, 12, n_bare=40, check=_is_peer_world)
    b = _synctest(o, n, 3, 12, n_bare=40)
    _compare(a, b, "follow 600")
    alive = a[1]["alive"]
    links = follow_links(n)
    assert (~alive).sum() > 20 and (~alive[links[links < n].astype(np.int64)]).any()       # entities died, and some link points at one of them
    assert (links >= n).sum() == 60
    moved = a[1]["c2w0"][alive] != 0                                                          # Vel.x of the living: the followers steer
    assert moved.any()


def test_follow_8300_slots_links_cross_the_layout_tile():
    n = 8300
    g, o = _pair(n + 32)
    a = _synctest(g, n, 2, 5, check=_is_peer_world)
    b = _synctest(o, n, 2, 5)
    _compare(a, b, "follow 8300")
    links = follow_links(n)
    i = np.arange(n)
    assert ((links < n) & ((links >> np.uint64(13)) != (i >> 13).astype(np.uint64))).any()   # a reader in one 8192-slot layout tile, its target in the other


def test_host_decided_spawns_children_and_links_to_slots_that_do_not_exist_yet():
    """Every fourth frame five children (ggrs_request::spawn_count, a user-written spawn system) that link to existing slots; before the session some older
    entities are relinked (upload_word) to the slots the children WILL take: such a link is !ok() until the frame after the spawn."""
    n = 300
    res = []
    for w in _pair(n + 128):
        ids = build_follow(w, with_spawn=True)
        spawn_follow(w, ids, n)
        future = (n + np.arange(12)).astype(np.uint64)                                       # the first 12 child slots
        w.upload_word(ids[1], 0, 20, future)
        drv = cm.SyncTestDriver(w, 2)
        for t in range(14):
            drv.tick((0,), patch=spawn_patch(n))
        res.append((drv.all_checksums, cm.snapshot_state(w, ids)))
    _compare(res[0], res[1], "follow with spawns")
    assert res[0][1]["len"] == n + sum(children(f, n)[0] for f in range(14)) > n + 12          # every frame that fires spawned its five; all 12 relinked slots exist by now


def _p2p_lists(ticks, seed=9):
    """[Load(F - k), (Advance, Save) x k] with k drawn 0..4 per tick, then the tick's new frame (Advance, Save): the world is at F with a snapshot of F."""
    rng = np.random.default_rng(seed)
    out, F = [], 0
    inp = lambda f: ((f * 7) & 3,)
    for _ in range(ticks):
        k = int(min(rng.integers(0, 5), F))
        reqs = [bg.LoadGameState(F - k)]
        for i in range(k + 1):
            reqs += [bg.AdvanceFrame(inp(F - k + i)), bg.SaveGameState(F - k + i + 1)]
        out.append((F, k, reqs))
        F += 1
    return out


def test_p2p_shaped_lists_two_in_flight():
    n = 700
    g, o = _pair(n + 16, depth=8)
    lists = _p2p_lists(14)
    got, want = [], []
    ids = build_follow(g); spawn_follow(g, ids, n, n_bare=30)
    g.set_depth(8); g.set_synctest_check_distance(-1)
    got += g.handle_requests([bg.SaveGameState(0)])
    inflight = 0
    for F, k, reqs in lists:
        if F - 8 >= 0: g.set_confirmed(F - 8)
        g.enqueue_requests(reqs); inflight += 1
        if inflight == 2: got += g.collect_checksums(); inflight -= 1
    while inflight: got += g.collect_checksums(); inflight -= 1
    _is_peer_world(g)
    ido = build_follow(o); spawn_follow(o, ido, n, n_bare=30)
    o.set_depth(8)
    want += o.handle_requests([bg.SaveGameState(0)])
    for F, k, reqs in lists:
        if F - 8 >= 0: o.set_confirmed(F - 8)
        for r in reqs: want += o.handle_requests([r])
    assert len(got) == len(want) == 1 + sum(k + 1 for _, k, _ in lists) and {k for _, k, _ in lists} == {0, 1, 2, 3, 4}
    assert got == want
    cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), "p2p-shaped lists")


VIS_SRC = r"""
// binding 0 = Seen (what the peer read returned: 0 when !ok()), 1 = Link, 2 = Fuse; peer binding 0 = Tag
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) {
    const GgrsPeer p = e.peer(e.u64(1));
    e.u32(0) = p.ok() ? p.u32(0) : 0u;
    if (e.u32(2) == 1u) e.despawn();                       // the reader despawns ITSELF in the frame its fuse says
    if (e.u32(2)) e.u32(2) -= 1u;
}
"""


def test_visibility_rule_in_isolation():
    """Four entities, expected values written by hand, no oracle.  Entity 1 despawns itself in frame 1 (its fuse is 1): entity 0, which links to it, still
    reads it in that frame -- Bevy's Commands are deferred -- and not in the next.  Entity 2 links out of range, entity 3 to itself."""
    w = bg.World(64, max_depth=4)
    S = w.register_component("Seen", 4, 1); L = w.register_component("Link", 8, 1); F = w.register_component("Fuse", 4, 1); T = w.register_component("Tag", 4, 1)
    w.checksum_component(S, [0])
    w.add_custom_system(VIS_SRC, [(S, 0), (L, 0), (F, 0)], name="look", peers=[(T, 0)])
    w.spawn(4, {S: [np.zeros(4, dtype=np.uint32)], L: [np.array([1, 0, 99, 3], dtype=np.uint64)], F: [np.array([0, 1, 0, 0], dtype=np.uint32)],
                T: [np.array([10, 11, 12, 13], dtype=np.uint32)]})
    seen = lambda: w.download_word(S, 0, 0, 4).tolist()
    w.handle_requests([bg.SaveGameState(0), bg.AdvanceFrame((0,))])              # frame 1: entity 1 despawns itself; everyone alive at the start of the frame is visible
    assert seen()[0] == 11 and seen()[2] == 0 and seen()[3] == 13, seen()
    assert w.alive_mask(4).tolist() == [True, False, True, True]
    w.handle_requests([bg.SaveGameState(1), bg.AdvanceFrame((0,))])              # frame 2: entity 1 is gone
    assert seen()[0] == 0 and seen()[2] == 0 and seen()[3] == 13, seen()
    w.handle_requests([bg.LoadGameState(1), bg.AdvanceFrame((0,))])              # the rollback re-simulates frame 2 from the snapshot: the same view
    assert seen()[0] == 0 and seen()[3] == 13, seen()
    w.handle_requests([bg.LoadGameState(0), bg.AdvanceFrame((0,))])              # ... and frame 1 from ITS snapshot: entity 1 is back, and visible
    assert seen()[0] == 11 and w.alive_mask(4).tolist() == [True, False, True, True], seen()


def test_every_frame_the_ring_holds_and_the_live_block():
    """After a session under the policies that would leave blocks unwritten (ggrs_dbg_set_lazy_live 3: every eligible list skips the live block and defers its
    Saves), nothing was deferred: the live block equals the oracle's as it stands, and every frame the ring holds loads to the oracle's."""
    n = 500
    g, o = _pair(n + 16)
    assert g._lib.ggrs_dbg_set_lazy_live(g._p, 3) == 0
    a = _synctest(g, n, 4, 10, n_bare=20)
    info = g.kernel_info()
    assert cm.deferred_counts(g) == (0, 0) and info["lazy_live_block"].startswith("off"), info     # (read BEFORE anything that would materialise)
    b = _synctest(o, n, 4, 10, n_bare=20)
    _compare(a, b, "live block")
    ids = (0, 1, 2, 3)
    frames = [f for f in range(g.frame + 1) if g.has_snapshot(f)]
    assert len(frames) >= 4 and frames == [f for f in range(o.frame + 1) if o.has_snapshot(f)]
    for f in reversed(frames):                                                                     # newest first: a Load pops the newer snapshots
        g.load(f); o.load(f)
        cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ids), f"ring frame {f}")


def test_specialised_copies_forced_at_first_sight(monkeypatch):
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    n = 400
    g, o = _pair(n + 16)
    assert g._lib.ggrs_dbg_set_spec_shapes(g._p, 3) == 0                                            # three places: the shapes of a SyncTest tick take turns
    spec = {}
    a = _synctest(g, n, 2, 8, n_bare=16, check=lambda w: spec.update(w.kernel_info()))
    b = _synctest(o, n, 2, 8, n_bare=16)
    assert spec["specialised_kernel"].startswith("ready"), spec["specialised_kernel"]
    _compare(a, b, "specialised copies")


def _fanout_rank(q, lib_path):
    try:
        os.environ["GGRS_RCCL_LIB"] = lib_path
        from bevy_ggrs_amd.fanout import RcclFanout
        n = 300
        g, o = _pair(n + 16)
        ids = build_follow(g); spawn_follow(g, ids, n)
        ido = build_follow(o); spawn_follow(o, ido, n)
        for w in (g, o): w.set_depth(6)
        native = RcclFanout(g, 0, 1, RcclFanout.unique_id())
        # ---- the compact branch form is refused ...
        pre, keep, _ = g.build_requests([bg.SaveGameState(0)])
        inputs = np.zeros((2, 2, 1), dtype=np.uint8)
        bs = _ffi.BranchStep()
        bs.prefix, bs.n_prefix, bs.n_branches, bs.n_frames, bs.n_inputs, bs.flags = pre, 1, 2, 2, 1, _ffi.BRANCH_SAVE_LAST
        bs.inputs = inputs.ctypes.data
        rc = _ffi.lib.ggrs_hip_fanout_step_branches(native._p, C.byref(bs), None)
        msg = (_ffi.lib.ggrs_hip_fanout_last_error(native._p) or b"").decode()
        # ---- ... the request-list form works: two branches off the snapshot of frame 0
        reqs = [bg.SaveGameState(0)]
        for b in range(2):
            reqs += [bg.LoadGameState(0), bg.AdvanceFrame((b + 1,)), bg.SaveGameState(1), bg.AdvanceFrame((b + 1,)), bg.SaveGameState(2)]
        ns = native.step(reqs)
        table = native.collect()
        got = [int(p[0]) | (int(p[1]) << 64) for p in table.reshape(-1, 2)]
        want = []
        for r in reqs: want += o.handle_requests([r])
        same = True
        try: cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), "fan-out")
        except AssertionError: same = False
        native.close()
        q.put(("ok", rc, msg, ns, got, want, same))
    except Exception as e:                                    # noqa: BLE001
        import traceback
        q.put(("error", f"{type(e).__name__}: {e}", traceback.format_exc()))


def test_branch_steps_are_refused_and_the_request_list_form_works():
    import multiprocessing as mp
    from test_gpu_zfanout import _double_lib                                                   # (a name only: no test is imported)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_fanout_rank, args=(q, _double_lib())); p.start()
    try: r = q.get(timeout=300)
    finally:
        p.join(timeout=60)
        if p.is_alive(): p.kill()
    assert r[0] == "ok", r
    _, rc, msg, ns, got, want, same = r
    assert rc == bg.GGRS_E_INVALID and "peer bindings" in msg and "ggrs_hip_fanout_step" in msg, (rc, msg)
    assert ns == 5 and got == want and same, (ns, got, want, same)
