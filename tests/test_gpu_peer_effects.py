"""Cross-entity writes for user-written systems (ggrs_hip_add_custom_system_effects): a system sends to the entity at a link -- a stable slot in an 8-byte word --
with e.send_u32 / e.send_i32 / e.send_u64, and every send of a frame lands at the END of the frame.  Everything goes through the C ABI and is bit-exact: the
Checksum(u128) of every SaveGameState, the final state and every frame the ring holds equal the CPU oracle's, whose callbacks compute a pass's effects from the
oracle's own columns and apply them last (peer_effects_common.py).

The reference lets a system take a second Query<&mut Health> and call get_mut(target); here a send is one relaxed no-return atomic into the world's inbox, and one
small launch right behind every request group that holds an AdvanceWorld combines the inbox into the live block.  Such a world's groups end on their one
AdvanceWorld.

Sessions: SyncTest, check distance 2, depth 8.  At n = 300 (links cross waves and the 256-slot workgroup) 40 ticks; at n = 9000 (links cross the 8192-slot layout
tile) 12 ticks = 36 simulated frames -- the oracle calls Python once per entity, system and frame, and 40 ticks of it take 12 s.  An oracle session is computed once
per shape and shared, unchanged, by the tests that compare against it."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
from bevy_ggrs_amd import _ffi
from oracle.binding import FLAT, OracleWorld
from peer_effects_common import Effects, build_strike, children, run_oracle, spawn_patch, spawn_strike, strike_links, synctest_lists

pytestmark = pytest.mark.gpu
CD, DEPTH = 2, 8
N_BARE = 12


def _relink_to_children(w, ids, n):
    """Some older entities link to the slots the first children WILL take: such a send is dropped until the frame after the spawn."""
    w.upload_word(ids[1], 0, 20, (n + np.arange(12)).astype(np.uint64))


def _setup(w, n, order, with_spawn, fx=None):
    ids = build_strike(w, order=order, with_spawn=with_spawn, **({"fx": fx} if fx is not None else {}))
    spawn_strike(w, ids, n, n_bare=N_BARE)
    if with_spawn: _relink_to_children(w, ids, n)
    w.set_depth(DEPTH)
    return ids


def _ring_states(w, ids):
    """Every frame the ring holds, loaded newest first (a Load pops the newer snapshots) and snapshotted."""
    frames = [f for f in range(w.frame + 1) if w.has_snapshot(f)]
    out = {}
    for f in reversed(frames):
        w.load(f)
        out[f] = cm.snapshot_state(w, ids)
    return out


@functools.lru_cache(maxsize=None)
def _reference(n, ticks, order="last", with_spawn=False):
    """The oracle's session: ([(frame, checksum)], final state, {frame: state} of the ring, the Effects record)."""
    o = OracleWorld(n + 128, DEPTH, FLAT)
    fx = Effects()
    ids = _setup(o, n, order, with_spawn, fx)
    lists = synctest_lists(CD, ticks, depth=DEPTH, patch=spawn_patch(n) if with_spawn else None)
    cks = run_oracle(o, lists, CD)
    final = cm.snapshot_state(o, ids)
    assert fx.landed * 2 > fx.sent > 0, (fx.landed, fx.sent)                  # more than half of all sends land: nothing passes by dropping everything
    return cks, final, _ring_states(o, ids), fx


def _is_effect_world(w, peers=False):
    info = w.kernel_info()
    assert info["request_group_kernel"].startswith("ggrs_jit_tick"), info
    assert info["group_caps"].endswith("/ 1 steps") and info["effect_inbox"].startswith("4 linear columns"), info
    assert info["lazy_live_block"].startswith("off") and info["deferred_saves"].startswith("off"), info
    assert ("peer_view" in info) == peers, info


def _gpu_session(n, ticks, *, order="last", with_spawn=False, how="handle", before=None):
    g = bg.World(n + 128, max_depth=DEPTH)
    ids = _setup(g, n, order, with_spawn)
    g.set_synctest_check_distance(CD)
    if before: before(g)
    lists = synctest_lists(CD, ticks, depth=DEPTH, patch=spawn_patch(n) if with_spawn else None)
    cks = []
    if how == "handle":
        for reqs in lists: cks += g.handle_requests(reqs)
    else:                                                                     # enqueue / collect, two lists in flight
        inflight = 0
        for reqs in lists:
            g.enqueue_requests(reqs); inflight += 1
            if inflight == 2: cks += g.collect_checksums(); inflight -= 1
        while inflight: cks += g.collect_checksums(); inflight -= 1
    frames = [r.frame for reqs in lists for r in reqs if isinstance(r, bg.SaveGameState)]
    return g, ids, list(zip(frames, cks))


def _compare(g, ids, cks, ref, ctx, ring=True):
    want, final, ring_states, _ = ref
    assert len(cks) == len(want) > 0, (len(cks), len(want))
    for (fa, ca), (fb, cb) in zip(cks, want):
        assert fa == fb and ca == cb, f"{ctx}: frame {fa}: gpu {ca:#x} oracle {cb:#x}"
    cm.assert_states_equal(cm.snapshot_state(g, ids), final, ctx)
    if not ring: return
    got = _ring_states(g, ids)
    assert sorted(got) == sorted(ring_states) and len(got) >= CD, (sorted(got), sorted(ring_states))
    for f in got: cm.assert_states_equal(got[f], ring_states[f], f"{ctx}: ring frame {f}")


@pytest.mark.parametrize("how", ["handle", "enqueue"])
@pytest.mark.parametrize("n,ticks", [(300, 40), (9000, 12)])
def test_strike_synctest_against_the_oracle(n, ticks, how):
    """Every frame's checksum, the final live state and every frame the ring holds; through ggrs_hip_handle_requests and through enqueue / collect."""
    ref = _reference(n, ticks)
    g, ids, cks = _gpu_session(n, ticks, how=how)
    _is_effect_world(g)
    _compare(g, ids, cks, ref, f"strike {n} {how}")
    final = ref[1]
    links = strike_links(n)
    i = np.arange(n)
    assert (~final["alive"]).sum() > 20 and (~final["alive"][links[links < n].astype(np.int64)]).any()      # entities died, and some link points at one of them
    assert (final["c3w0"] > 0x80000000).any()                                                             # an Hp wrapped below zero
    assert (final["c6w0"][final["alive"]] >> np.uint64(32) != (i.astype(np.uint64)[final["alive"]] << np.uint64(1))).any()   # Score took adds above 2^32
    if n > 8192: assert ((links < n) & ((links >> np.uint64(13)) != (i >> 13).astype(np.uint64))).any()    # a sender in one 8192-slot layout tile, its target in the other


def test_host_decided_spawns_children_are_not_hit_in_their_first_frame():
    """Every fourth frame five children (ggrs_request::spawn_count, a user-written spawn system) that link to existing slots and strike from their second frame on;
    before the session some older entities are relinked to the slots the children WILL take: such a send is dropped until the frame after the spawn."""
    n, ticks = 300, 16
    ref = _reference(n, ticks, with_spawn=True)
    g, ids, cks = _gpu_session(n, ticks, with_spawn=True)
    _compare(g, ids, cks, ref, "strike with spawns")
    assert ref[1]["len"] == n + sum(children(f, n)[0] for f in range(ticks)) > n + 12           # every frame that fires spawned its five; all 12 relinked slots exist by now
    flags = ref[1]["c4w0"][n:n + 12]
    assert flags.any()                                                                         # ... and were hit once they existed


def test_p2p_shaped_lists_whose_rollback_length_varies():
    """[Load(F - k), (Advance, Save) x (k + 1)] with k drawn 0..4 per tick, two lists in flight."""
    n = 300
    rng = np.random.default_rng(9)
    lists, F = [], 0
    for _ in range(14):
        k = int(min(rng.integers(0, 5), F))
        reqs = [bg.LoadGameState(F - k)]
        for i in range(k + 1): reqs += [bg.AdvanceFrame((((F - k + i) * 7) & 3,)), bg.SaveGameState(F - k + i + 1)]
        lists.append((F, k, reqs)); F += 1
    assert {k for _, k, _ in lists} == {0, 1, 2, 3, 4}
    g = bg.World(n + 128, max_depth=DEPTH); ids = _setup(g, n, "last", False); g.set_synctest_check_distance(-1)
    o = OracleWorld(n + 128, DEPTH, FLAT); ido = _setup(o, n, "last", False)
    got = g.handle_requests([bg.SaveGameState(0)]); want = o.handle_requests([bg.SaveGameState(0)])
    inflight = 0
    for F, k, reqs in lists:
        if F - 8 >= 0: g.set_confirmed(F - 8)
        g.enqueue_requests(reqs); inflight += 1
        if inflight == 2: got += g.collect_checksums(); inflight -= 1
    while inflight: got += g.collect_checksums(); inflight -= 1
    for F, k, reqs in lists:
        if F - 8 >= 0: o.set_confirmed(F - 8)
        for r in reqs: want += o.handle_requests([r])
    assert len(got) == len(want) == 1 + sum(k + 1 for _, k, _ in lists)
    assert got == want
    cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), "p2p-shaped lists")


RULES_SRC = r"""
// binding 0 = Link, 1 = Fuse; effect binding 0 = Hp (ADD), 1 = Mark (MAX_U).  An entity whose fuse is 1 despawns itself in this frame -- and still sends
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) {
    e.send_u32(e.u64(0), 0, 0u - 3u);
    e.send_u32(e.u64(0), 1, (ggrs_u32)e.slot + 10u);
    e.send_u64(e.u64(0), 0, 99ull);                        // the wrong width for a 4-byte column: dropped
    if (e.u32(1) == 1u) e.despawn();
    if (e.u32(1)) e.u32(1) -= 1u;
}
"""


def _rules_world():
    w = bg.World(64, max_depth=4)
    L = w.register_component("Link", 8, 1); F = w.register_component("Fuse", 4, 1); H = w.register_component("Hp", 4, 1); M = w.register_component("Mark", 4, 1)
    w.checksum_component(H, [0]); w.checksum_component(M, [0])
    w.add_custom_system(RULES_SRC, [(L, 0), (F, 0)], name="striker", effects=[(H, 0, bg.EFFECT_ADD), (M, 0, bg.EFFECT_MAX_U)])
    # slot:   0 -> 1      1 -> 0 (dies in frame 1)      2 -> 99 (out of range)      3 -> 3 (itself)      4 -> 5 (no Hp)      5 -> 0
    link = np.array([1, 0, 99, 3, 5, 0], dtype=np.uint64); fuse = np.array([0, 1, 0, 0, 0, 0], dtype=np.uint32)
    w.spawn(5, {L: [link[:5]], F: [fuse[:5]], H: [np.array([10, 20, 30, 2, 50], dtype=np.uint32)], M: [np.zeros(5, dtype=np.uint32)]})
    w.spawn(1, {L: [link[5:]], F: [fuse[5:]], M: [np.zeros(1, dtype=np.uint32)]})                # slot 5 has no Hp
    return w, (L, F, H, M)


def test_send_rules_in_isolation_and_an_immediate_download():
    """Six entities, expected values written by hand, no oracle.  The list ENDS on its AdvanceWorld and the download follows at once: it shows the effects."""
    w, (L, F, H, M) = _rules_world()
    hp = lambda: w.download_word(H, 0, 0, 6).tolist(); mark = lambda: w.download_word(M, 0, 0, 6).tolist()
    w.handle_requests([bg.SaveGameState(0), bg.AdvanceFrame((0,))])
    # frame 1: 0 takes -3 from 1 AND -3 from 5 (the sender 1 despawns itself in the same call and still sends); 1 is despawned in this frame: the send of 0 is dropped;
    # 2 sends out of range; 3 hits itself and wraps below zero; 5 has no Hp: the Hp send of 4 is dropped, its Mark send lands
    assert w.alive_mask(6).tolist() == [True, False, True, True, True, True]
    h = hp(); m = mark()
    assert h[0] == 10 - 6 and h[2] == 30 and h[3] == (2 - 3) & 0xFFFFFFFF and h[4] == 50, h
    assert m[0] == 15 and m[2] == 0 and m[3] == 13 and m[4] == 0 and m[5] == 14, m
    assert w.download_word(H, 0, 1, 1)[0] == 20                       # (the dead entity's word was not touched)
    w.handle_requests([bg.SaveGameState(1), bg.AdvanceFrame((0,))])
    # frame 2: 1 is gone -- it neither sends nor receives; 0 takes -3 from 5 only
    h = hp()
    assert h[0] == 10 - 6 - 3 and h[3] == (2 - 6) & 0xFFFFFFFF, h
    w.handle_requests([bg.LoadGameState(1), bg.AdvanceFrame((0,))])   # the rollback re-simulates frame 2 from the snapshot: the same effects, once
    assert hp()[0] == 10 - 6 - 3 and hp()[3] == (2 - 6) & 0xFFFFFFFF, hp()
    w.handle_requests([bg.LoadGameState(0), bg.AdvanceFrame((0,))])   # ... and frame 1 from ITS snapshot
    assert hp()[0] == 10 - 6 and hp()[3] == (2 - 3) & 0xFFFFFFFF and mark()[0] == 15, (hp(), mark())
    # the blocking API: one AdvanceWorld, then a SaveWorld whose checksum covers the effects
    w.advance()
    a = w.save()
    assert hp()[0] == 10 - 6 - 3
    w.load(w.frame)
    assert w.save() == a


def test_the_inbox_holds_identities_after_a_session():
    """Inferred: after a session, an idle frame with every link out of range leaves the four effect columns unchanged (a word left in the inbox would be applied by
    that frame's apply launch)."""
    n = 300
    g, ids, _ = _gpu_session(n, 10)
    g.upload_word(ids[1], 0, 0, np.full(n, n + 5, dtype=np.uint64))
    cols = lambda: [g.download_word(c, 0, 0, n).tolist() for c in ids[3:]]
    before = cols()
    g.handle_requests([bg.AdvanceFrame((0,))])
    g.handle_requests([bg.AdvanceFrame((0,))])
    assert cols() == before
    assert int(g.kernel_info()["effect_inbox"].split("(")[1].split()[0]) > 10          # the applies ran


def test_peer_reads_and_effects_in_one_system():
    """The striker is registered FIRST, peer-reads its target's Pos.x (the start of the frame) and sends it damage that depends on it."""
    n, ticks = 300, 16
    ref = _reference(n, ticks, order="first")
    g, ids, cks = _gpu_session(n, ticks, order="first")
    _is_effect_world(g, peers=True)
    _compare(g, ids, cks, ref, "peers + effects")


def test_specialised_copies_forced_at_first_sight(monkeypatch):
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    n, ticks = 300, 40
    ref = _reference(n, ticks)
    g, ids, cks = _gpu_session(n, ticks, before=lambda w: w._lib.ggrs_dbg_set_spec_shapes(w._p, 3))
    assert g.kernel_info()["specialised_kernel"].startswith("ready"), g.kernel_info()["specialised_kernel"]
    _compare(g, ids, cks, ref, "specialised copies")


def _fanout_rank(q, lib_path):
    try:
        os.environ["GGRS_RCCL_LIB"] = lib_path
        from bevy_ggrs_amd.fanout import RcclFanout
        n = 300
        g = bg.World(n + 128, max_depth=6); o = OracleWorld(n + 128, 6, FLAT)
        ids = build_strike(g); spawn_strike(g, ids, n, n_bare=N_BARE)
        ido = build_strike(o); spawn_strike(o, ido, n, n_bare=N_BARE)
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
    assert rc == bg.GGRS_E_INVALID and "effect bindings" in msg and "ggrs_hip_fanout_step" in msg, (rc, msg)
    assert ns == 5 and got == want and same, (ns, got, want, same)
