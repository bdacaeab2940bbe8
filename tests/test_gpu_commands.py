"""Structural commands in user-written systems (ggrs_hip_add_custom_system_commands): a system inserts and removes components of its OWN entity -- e.has(j),
e.opt_*(j, k), e.insert(j), e.remove(j) -- inside the generated kernel, so that a rollback replays them.  Everything goes through the C ABI and is bit-exact: the
Checksum(u128) of every SaveGameState, the final state (alive, every presence mask ANDed with alive and cut at len, every word of every present component) and
every frame the ring holds equal the CPU oracle's, whose callbacks edit the oracle world directly (commands_common.py).

Every reference asserts on the ORACLE side that inserts, removes and writes in place each happened at least once per simulated frame on average, and that the
final presence count is neither 0 nor len: otherwise a test would prove nothing.

Shapes: 130 slots (two full waves and a 2-lane tail in one mask word), 300 (crosses the 256-slot workgroup), 8262 (crosses the 8192-slot layout tile; 12 ticks at
check distance 2 -- the oracle calls Python once per entity and frame, and check distance 7 there would be 800 k calls).  An oracle session is computed once per
shape and shared, unchanged, by the tests that compare against it."""
import ctypes as C
import functools

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
from bevy_ggrs_amd import _ffi
from commands_common import (BOTH, Counts, build_shield, build_stun, build_watch, run_oracle, spawn_shield, spawn_stun, spawn_watch, synctest_lists)
from oracle.binding import FLAT, OracleWorld

pytestmark = pytest.mark.gpu
DEPTH = 8
WORLDS = {"stun": (build_stun, spawn_stun), "shield": (build_shield, spawn_shield), "watch": (build_watch, spawn_watch)}


def _inputs(t): return (t % 3,)


def _spawn_patch(frame, r):
    """The host side of the spawn system, a pure function of the frame: in every fourth frame five children."""
    if frame % 4 == 1: r.spawn_count = 5


def _setup(w, world, n, cnt=None, **kw):
    build, spawn = WORLDS[world]
    ids = build(w, **({"cnt": cnt} if isinstance(w, OracleWorld) else {}), **kw)
    spawn(w, ids, n)
    w.set_depth(DEPTH)
    return ids


def _ring_states(w, ids):
    """Every frame the ring holds, loaded newest first (a Load pops the newer snapshots) and snapshotted."""
    out = {}
    for f in reversed([f for f in range(w.frame + 1) if w.has_snapshot(f)]):
        w.load(f)
        out[f] = cm.snapshot_state(w, ids)
    return out


def _busy(cnt, lists, final, comp, ctx):
    """The oracle's session did what the test is about."""
    frames = sum(isinstance(r, bg.AdvanceFrame) for reqs in lists for r in reqs)
    assert min(cnt.inserts, cnt.removes, cnt.writes) >= frames > 0, (ctx, cnt.inserts, cnt.removes, cnt.writes, frames)
    assert 0 < int(final[f"present{comp}"].sum()) < final["len"], (ctx, int(final[f"present{comp}"].sum()), final["len"])


@functools.lru_cache(maxsize=None)
def _reference(world, n, cd, ticks, spawn=None, kills=False):
    """The oracle's session: ([(frame, checksum)], final state, {frame: state} of the ring)."""
    o = OracleWorld(n + 128, DEPTH, FLAT)
    cnt = Counts()
    kw = {"spawn": spawn, "kills": kills} if world == "stun" else {}
    ids = _setup(o, world, n, cnt, **kw)
    lists = synctest_lists(cd, ticks, depth=DEPTH, patch=_spawn_patch if spawn else None, inputs=_inputs)
    cks = run_oracle(o, lists, cd)
    final = cm.snapshot_state(o, ids)
    _busy(cnt, lists, final, ids[-1], (world, n, cd))
    return cks, final, _ring_states(o, ids)


def _gpu_session(world, n, cd, ticks, *, spawn=None, kills=False, before=None, cap=None):
    g = bg.World(cap or n + 128, max_depth=DEPTH)
    if before: before(g)
    kw = {"spawn": spawn, "kills": kills} if world == "stun" else {}
    ids = _setup(g, world, n, **kw)
    g.set_synctest_check_distance(cd)
    lists = synctest_lists(cd, ticks, depth=DEPTH, patch=_spawn_patch if spawn else None, inputs=_inputs)
    cks = []
    for reqs in lists: cks += g.handle_requests(reqs)
    frames = [r.frame for reqs in lists for r in reqs if isinstance(r, bg.SaveGameState)]
    return g, ids, list(zip(frames, cks))


def _compare(g, ids, cks, ref, ctx, cd):
    want, final, ring_states = ref
    assert len(cks) == len(want) > 0, (len(cks), len(want))
    for (fa, ca), (fb, cb) in zip(cks, want):
        assert fa == fb and ca == cb, f"{ctx}: frame {fa}: gpu {ca:#x} oracle {cb:#x}"
    cm.assert_states_equal(cm.snapshot_state(g, ids), final, ctx)
    got = _ring_states(g, ids)
    assert sorted(got) == sorted(ring_states) and len(got) >= min(cd, 2), (sorted(got), sorted(ring_states))
    for f in got: cm.assert_states_equal(got[f], ring_states[f], f"{ctx}: ring frame {f}")


def _is_command_world(g):
    """Every policy stays on for such a world, as for a fused-spawn world: nothing was switched off to make it pass."""
    info = g.kernel_info()
    assert info["request_group_kernel"].startswith("ggrs_jit_tick"), info
    assert "live-only state" not in info["lazy_live_block"] and info["deferred_saves"].startswith("on"), info        # (not switched off by a policy function)
    assert not info["group_caps"].endswith("/ 1 steps") and info["command_bindings"].startswith("1 components"), info


@pytest.mark.parametrize("n,cd,ticks", [(130, 2, 40), (130, 7, 24), (300, 2, 40), (300, 7, 24), (8262, 2, 12)])
def test_stun_synctest_against_the_oracle(n, cd, ticks):
    ref = _reference("stun", n, cd, ticks)
    g, ids, cks = _gpu_session("stun", n, cd, ticks)
    _is_command_world(g)
    _compare(g, ids, cks, ref, f"stun {n} cd {cd}", cd)
    if n > 8192: assert ref[1]["present1"][8192:].any() and ref[1]["present1"][:8192].any()       # Stun on both sides of the layout tile's edge


@pytest.mark.parametrize("n,cd,ticks", [(130, 2, 40), (300, 7, 24)])
def test_shield_flags0_binding_eight_byte_word_earlier_and_later_systems(n, cd, ticks):
    """absorb writes Shield through a flags-0 binding (Option<&mut C>); tally, registered LATER, runs in the same frame for an entity the granter just gave a
    Shield; drain, registered EARLIER, from the next frame on."""
    ref = _reference("shield", n, cd, ticks)
    g, ids, cks = _gpu_session("shield", n, cd, ticks)
    _compare(g, ids, cks, ref, f"shield {n} cd {cd}", cd)
    charge = ref[1]["c1w0"][ref[1]["present1"]]
    assert (charge > np.uint64(1 << 32)).all() and len(set((charge >> np.uint64(32)).tolist())) > 2          # 8-byte words, used above 2^32


@pytest.mark.parametrize("spawn", ["with", "without"])
def test_fused_spawn_system_whose_bundle_includes_and_excludes_stun(spawn):
    n, cd, ticks = 300, 2, 24
    ref = _reference("stun", n, cd, ticks, spawn=spawn)
    g, ids, cks = _gpu_session("stun", n, cd, ticks, spawn=spawn)
    _compare(g, ids, cks, ref, f"stun, children {spawn} Stun", cd)
    assert ref[1]["len"] > n + 20
    if spawn == "with": assert (ref[1]["c1w1"][n:][ref[1]["present1"][n:]] == 77).any()           # a child's seed: the registered default, until its first own insert


def test_insert_and_despawn_in_the_same_call():
    n, cd, ticks = 300, 2, 40
    ref = _reference("stun", n, cd, ticks, kills=True)
    g, ids, cks = _gpu_session("stun", n, cd, ticks, kills=True)
    _compare(g, ids, cks, ref, "stun with kills", cd)
    dead = ~ref[1]["alive"]
    assert dead.sum() >= 5 and (np.nonzero(dead)[0] % 29 == 7).all()
    # the command applied although the call despawned the entity: the dead slot's presence bit is set, its words are what the call inserted
    pres = g.present_mask(ids[1], n)
    assert pres[dead].all() and (g.download_word(ids[1], 0, 0, n)[dead] == 3).all()


def _p2p_lists(ticks, seed, kmax):
    rng = np.random.default_rng(seed)
    lists, F = [], 0
    for t in range(ticks):
        k = int(min(t % (kmax + 1) if t < 2 * (kmax + 1) else rng.integers(0, kmax + 1), F))
        reqs = [bg.LoadGameState(F - k)]
        for i in range(k + 1): reqs += [bg.AdvanceFrame(_inputs(F - k + i)), bg.SaveGameState(F - k + i + 1)]
        lists.append((F, k, reqs)); F += 1
    return lists


def test_host_spawns_between_lists_then_p2p_shaped_rollbacks_of_0_to_7_frames():
    """[Save(F), Advance] lists with ggrs_hip_spawn between them (the new entities have no Stun; they gain it in the session); then [Load(F - k), (Advance, Save) x
    (k + 1)] with k = 0..7, two lists in flight."""
    n, depth = 300, 10
    worlds = []
    for w in (bg.World(n + 128, max_depth=depth), OracleWorld(n + 128, depth, FLAT)):
        cnt = Counts()
        ids = build_stun(w, **({"cnt": cnt} if isinstance(w, OracleWorld) else {})); spawn_stun(w, ids, n); w.set_depth(depth)
        worlds.append((w, ids, cnt))
    (g, ids, _), (o, ido, cnt) = worlds
    g.set_synctest_check_distance(-1)
    got, want, F0 = [], [], 6
    for f in range(F0):
        reqs = [bg.SaveGameState(f), bg.AdvanceFrame(_inputs(f))]
        got += g.handle_requests(reqs)
        for r in reqs: want += o.handle_requests([r])
        if f in (1, 3):
            for w, wi, _ in worlds: w.spawn(7, {wi[0]: [(np.arange(7) * 5 + f).astype(np.uint32)]})
    lists = [(F + F0, k, [type(r)(r.frame + F0) if not isinstance(r, bg.AdvanceFrame) else r for r in reqs]) for F, k, reqs in _p2p_lists(30, 4, 7)]
    lists[0] = (F0, 0, [bg.SaveGameState(F0), bg.AdvanceFrame(_inputs(F0)), bg.SaveGameState(F0 + 1)])          # (frame F0 has no snapshot yet)
    assert {k for _, k, _ in lists} == set(range(8))
    inflight = 0
    for F, k, reqs in lists:
        if F - depth >= 0: g.set_confirmed(F - depth)
        g.enqueue_requests(reqs); inflight += 1
        if inflight == 2: got += g.collect_checksums(); inflight -= 1
    while inflight: got += g.collect_checksums(); inflight -= 1
    for F, k, reqs in lists:
        if F - depth >= 0: o.set_confirmed(F - depth)
        for r in reqs: want += o.handle_requests([r])
    assert len(got) == len(want) == F0 + 1 + sum(k + 1 for _, k, _ in lists)
    assert got == want
    final = cm.snapshot_state(o, ido)
    cm.assert_states_equal(cm.snapshot_state(g, ids), final, "p2p-shaped lists")
    assert final["len"] == n + 14 and final["present1"][n:].any()
    _busy(cnt, [r for _, _, r in lists], final, ido[1], "p2p")
    rg, ro = _ring_states(g, ids), _ring_states(o, ido)
    assert sorted(rg) == sorted(ro) and len(rg) >= 8
    for f in rg: cm.assert_states_equal(rg[f], ro[f], f"p2p ring frame {f}")


def test_knob_every_group_defers_its_saves_and_leaves_the_live_block():
    n, cd, ticks = 300, 2, 40
    g, ids, cks = _gpu_session("stun", n, cd, ticks, before=lambda w: w._lib.ggrs_dbg_set_lazy_live(w._p, 3))
    d = cm.deferred_counts(g)
    assert d is not None and d[0] > ticks // 2, (d, g.kernel_info()["deferred_saves"])           # the knob took: Saves were deferred ...
    _compare(g, ids, cks, _reference("stun", n, cd, ticks), "lazy live 3", cd)
    assert cm.deferred_counts(g)[1] > 0, g.kernel_info()["deferred_saves"]                       # ... and the ring frames just compared were replayed on demand


def test_knob_value_tags_on():
    n, cd, ticks = 300, 2, 40
    g, ids, cks = _gpu_session("stun", n, cd, ticks, before=lambda w: w._lib.ggrs_dbg_set_value_tags(w._p, 1))
    assert g.kernel_info()["value_tags"].startswith("on"), g.kernel_info()["value_tags"]
    _compare(g, ids, cks, _reference("stun", n, cd, ticks), "value tags", cd)


def test_knob_specialised_copies_forced_at_first_sight(monkeypatch):
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    n, cd, ticks = 300, 2, 40
    g, ids, cks = _gpu_session("stun", n, cd, ticks, before=lambda w: w._lib.ggrs_dbg_set_spec_shapes(w._p, 3))
    assert g.kernel_info()["specialised_kernel"].startswith("ready"), g.kernel_info()["specialised_kernel"]
    _compare(g, ids, cks, _reference("stun", n, cd, ticks), "specialised copies", cd)


def test_lane_fold_path_checksums_do_not_depend_on_capacity():
    """The same 2000 entities in a world of capacity 4096 (the wave ladder) and of 98 304 (JIT_LANE_FOLD_MIN_SLOTS: per-lane LDS rows); the small one against the oracle."""
    n, cd, ticks = 2000, 2, 8
    ref = _reference("stun", n, cd, ticks)
    small = _gpu_session("stun", n, cd, ticks, cap=4096)
    big = _gpu_session("stun", n, cd, ticks, cap=98304)
    assert "s_lane" in big[0].generated_kernel_source() and "s_lane" not in small[0].generated_kernel_source()
    assert [c for _, c in big[2]] == [c for _, c in small[2]]
    _compare(small[0], small[1], small[2], ref, "capacity 4096", cd)
    _compare(big[0], big[1], big[2], ref, "capacity 98304", cd)


def test_peer_read_of_a_component_a_later_system_inserts():
    """watcher (registered first) peer-reads Stun.ticks of its target; the stun system, registered later, inserts and removes Stun: ok() follows the presence at
    the START of the frame."""
    n, cd, ticks = 300, 2, 16
    ref = _reference("watch", n, cd, ticks)
    g, ids, cks = _gpu_session("watch", n, cd, ticks)
    assert "peer_view" in g.kernel_info()
    _compare(g, ids, cks, ref, "peers + commands", cd)
    seen = ref[1]["c1w0"]
    assert (seen % 100 != 0).any() and (seen >= 100).any()                                       # some reads were ok(), some were not


RULES_SRC = r"""
// binding 0 = Hp; command binding 0 = Buff {a, b} (default {5, 6}), INSERT | REMOVE
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    switch (e.u32(0)) {
    case 1: e.opt_u32(0, 0) = 40u; e.insert(0); break;                   // absent: word 1 keeps the default; present: replaces word 0, keeps word 1
    case 2: e.insert(0); e.remove(0); break;                             // the last call wins: gone
    case 3: e.remove(0); e.opt_u32(0, 1) = 9u; e.insert(0); break;       // ... here: stays, written
    case 4: e.opt_u32(0, 0) = 99u; break;                                // a write without a command: lands only where the component is present
    default: break;
    }
    e.u32(0) = e.u32(0) + 10u * (e.has(0) ? 1u : 0u);                    // has() follows this call's own commands
}
"""


def test_command_rules_in_isolation():
    """Eight entities, expected values written by hand, no oracle: hp 1..4, each once without and once with Buff {20, 21}."""
    w = bg.World(64, max_depth=4)
    H = w.register_component("Hp", 4, 1); B = w.register_component("Buff", 4, 2)
    w.set_component_default(B, np.array([5, 6], dtype=np.uint32))
    w.checksum_component(H, [0]); w.checksum_component(B, [0, 1])
    w.add_custom_system(RULES_SRC, [(H, 0)], name="rules", commands=[(B, BOTH)])
    hp = np.array([1, 2, 3, 4], dtype=np.uint32)
    w.spawn(4, {H: [hp]})
    w.spawn(4, {H: [hp], B: [np.full(4, 20, dtype=np.uint32), np.full(4, 21, dtype=np.uint32)]})
    a = w.handle_requests([bg.SaveGameState(0), bg.AdvanceFrame((0,)), bg.SaveGameState(1)])
    pres = w.present_mask(B, 8).tolist()
    b0, b1, h = (w.download_word(B, 0, 0, 8).tolist(), w.download_word(B, 1, 0, 8).tolist(), w.download_word(H, 0, 0, 8).tolist())
    assert pres == [True, False, True, False, True, False, True, True], pres
    assert (b0[0], b1[0]) == (40, 6) and (b0[2], b1[2]) == (5, 9)                                # inserted on an absent entity: the defaults where the call wrote nothing
    assert (b0[4], b1[4]) == (40, 21) and (b0[6], b1[6]) == (20, 9) and (b0[7], b1[7]) == (99, 21)
    assert h == [11, 2, 13, 4, 11, 2, 13, 14], h
    # a rollback re-simulates the frame from the snapshot: the same commands, the same checksum
    b = w.handle_requests([bg.LoadGameState(0), bg.AdvanceFrame((0,)), bg.SaveGameState(1)])
    assert a[1] == b[0] and a[0] != a[1]
    assert w.present_mask(B, 8).tolist() == pres
    w.load(0)
    assert w.present_mask(B, 8).tolist() == [False] * 4 + [True] * 4 and w.download_word(H, 0, 0, 8).tolist() == [1, 2, 3, 4] * 2


def _fanout_rank(q, lib_path):
    try:
        import os
        os.environ["GGRS_RCCL_LIB"] = lib_path
        import branch_marks_common as bm
        from bevy_ggrs_amd.fanout import RcclFanout
        n, depth, B, T, F = 300, 8, 8, 4, 3
        g = bg.World(n + 128, max_depth=depth); o = OracleWorld(n + 128, depth, FLAT)
        cnt = Counts()
        ids = build_stun(g); spawn_stun(g, ids, n)
        ido = build_stun(o, cnt=cnt); spawn_stun(o, ido, n)
        for w in (g, o):
            w.set_depth(depth)
            for f in range(F): w.handle_requests([bg.SaveGameState(f), bg.AdvanceFrame(_inputs(f))])          # some entities are stunned when the branches start
        native = RcclFanout(g, 0, 1, RcclFanout.unique_id())
        pred = (np.arange(B)[:, None] * 3 + np.arange(T)[None, :] * 5) % 7                          # input-dependent inserts: the branches diverge in presence
        prefix = [bg.SaveGameState(F)]
        rc_keep, msg = bm.library_step(native, g, prefix, pred, _ffi.BRANCH_SAVE_LAST | _ffi.BRANCH_RETAIN_ALL)
        rc, got = bm.library_step(native, g, prefix, pred, _ffi.BRANCH_SAVE_LAST)
        reqs = list(prefix)
        for b in range(B): reqs += bm.branch_requests(F, pred[b], T, True, T)
        reqs.append(bg.LoadGameState(F))
        ns = native.step(reqs)
        table = native.collect()
        listed = [int(p[0]) | (int(p[1]) << 64) for p in table.reshape(-1, 2)]
        pres0 = int((g.present_mask(ids[1], n) & g.alive_mask(n)).sum())
        want = bm.oracle_walk(o, prefix, F, pred, True)
        same = True
        try: cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), "fan-out")
        except AssertionError: same = False
        native.close()
        q.put(("ok", rc_keep, msg, rc, got, ns, listed, want, same, pres0, (cnt.inserts, cnt.removes, cnt.writes)))
    except Exception as e:                                    # noqa: BLE001
        import traceback
        q.put(("error", f"{type(e).__name__}: {e}", traceback.format_exc()))


def test_branch_steps_without_retention_equal_the_request_list_form():
    """ggrs_hip_fanout_step_branches, 8 branches x 4 frames off one snapshot (a member's presence bits live in registers), against ggrs_hip_fanout_step's list form
    on the same world and the oracle's walk; GGRS_BRANCH_RETAIN_ALL is refused."""
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
    _, rc_keep, msg, rc, got, ns, listed, want, same, pres0, counts = r
    assert rc_keep == bg.GGRS_E_INVALID and "GGRS_BRANCH_RETAIN_" in msg and "command bindings" in msg, (rc_keep, msg)
    assert rc == 0 and len(got) == 1 and len(got[0]) == 1 + 8 * 4, (rc, got)
    assert ns == 1 + 8 * 4 and got[0] == listed == want, (ns, got, listed, want)
    assert len({tuple(got[0][1 + 4 * b: 5 + 4 * b]) for b in range(8)}) >= 6                    # the branches diverge
    assert same and 0 < pres0 < 300 and min(counts) > 0, (same, pres0, counts)
