"""Remote structural commands (ggrs_hip_add_custom_system_remote): a user-written system despawns OTHER entities and inserts / removes their components --
e.send_despawn(slot), e.send_insert(slot, j), e.send_remove(slot, j) -- through one inbox word per slot and k_apply_remote behind every request group that holds an
AdvanceWorld.  Everything goes through the C ABI and is bit-exact: the Checksum(u128) of every SaveGameState, the final state (alive, every presence mask ANDed
with alive and cut at len, every word of every present component) and every frame the ring holds equal the CPU oracle's, whose apply callback mirrors the
end-of-frame rules (remote_commands_common.py).  The oracle sessions are the ones test_remote_commands_text.py holds to the coverage floors -- inserts on absent and
on present components, removes, despawns, both conflicts, every kind of dropped command --, computed once per scenario and shared, unchanged.

Shapes: 200 slots (one workgroup, a ragged tail unit), 8300 (links cross 64-slot units, 256-slot workgroups and the 8192-slot layout tile; 10 ticks at check
distance 2 -- the oracle calls Python once per entity, system and frame)."""
import ctypes as C
import os

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
from bevy_ggrs_amd import _ffi
from oracle.binding import FLAT, OracleWorld
from remote_commands_common import build_hit, p2p_lists, spawn_hit, strike_links
from test_remote_commands_text import DEPTH, SCENARIOS, oracle_session, scenario_lists      # (names only: the scenarios and their cached oracle sessions)

pytestmark = pytest.mark.gpu


def _ring_states(w, ids):
    """Every frame the ring holds, loaded newest first (a Load pops the newer snapshots) and snapshotted."""
    out = {}
    for f in reversed([f for f in range(w.frame + 1) if w.has_snapshot(f)]):
        w.load(f)
        out[f] = cm.snapshot_state(w, ids)
    return out


_REF_RINGS = {}


def _reference(name):
    """(checksums, final state, {frame: state} of the oracle's ring) of a scenario; the ring is walked once (it rewinds the oracle world) and kept."""
    cks, final, o, ids, st = oracle_session(name)
    if name not in _REF_RINGS: _REF_RINGS[name] = _ring_states(o, ids)
    return cks, final, _REF_RINGS[name]


def _gpu_world(name, before=None, remote=True):
    n, cd, ticks, kw = SCENARIOS[name]
    g = bg.World(n + 128, max_depth=DEPTH)
    if before: before(g)
    ids = build_hit(g, remote=remote, **kw); spawn_hit(g, ids, n); g.set_depth(DEPTH)
    g.set_synctest_check_distance(cd)
    return g, ids


def _gpu_session(name, before=None):
    g, ids = _gpu_world(name, before)
    lists = scenario_lists(name)
    cks = []
    for reqs in lists: cks += g.handle_requests(reqs)
    frames = [r.frame for reqs in lists for r in reqs if isinstance(r, bg.SaveGameState)]
    return g, ids, list(zip(frames, cks)), lists


def _compare(g, ids, cks, ref, ctx):
    want, final, ring_states = ref
    assert len(cks) == len(want) > 0, (len(cks), len(want))
    for (fa, ca), (fb, cb) in zip(cks, want):
        assert fa == fb and ca == cb, f"{ctx}: frame {fa}: gpu {ca:#x} oracle {cb:#x}"
    cm.assert_states_equal(cm.snapshot_state(g, ids), final, ctx)
    got = _ring_states(g, ids)
    assert sorted(got) == sorted(ring_states) and len(got) >= 2, (sorted(got), sorted(ring_states))
    for f in got: cm.assert_states_equal(got[f], ring_states[f], f"{ctx}: ring frame {f}")


def _inbox(g):
    """The remote inbox as the device holds it once everything queued has run (ggrs_dbg_remote_inbox)."""
    g._lib.ggrs_dbg_remote_inbox.restype = C.c_int64
    g._lib.ggrs_dbg_remote_inbox.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    buf = np.full(1 << 16, 0xA5A5A5A5, dtype=np.uint32)
    n = g._lib.ggrs_dbg_remote_inbox(g._p, buf.ctypes.data, buf.nbytes)
    assert 0 < n <= buf.nbytes and n % 4 == 0, n
    return buf[:n // 4]


def _applies(g):
    info = g.kernel_info()
    return int(info["remote_inbox"].split("(")[-1].split(" applies")[0]), info


def _is_remote_world(g, lists, peers=False):
    n_adv = sum(isinstance(r, bg.AdvanceFrame) for reqs in lists for r in reqs)
    applies, info = _applies(g)
    assert info["request_group_kernel"].startswith("ggrs_jit_tick"), info
    assert info["group_caps"].endswith("/ 1 steps") and info["remote_inbox"].startswith("one u32 per slot, 2 remotely commanded components"), info
    assert info["lazy_live_block"].startswith("off") and info["deferred_saves"].startswith("off"), info
    assert ("peer_view" in info) == peers, info
    assert applies == n_adv > 0, (applies, n_adv)                            # one apply per AdvanceWorld executed
    assert not _inbox(g).any()                                               # the invariant: all zeros whenever no group-and-apply pair is in flight


@pytest.mark.parametrize("name", ["200 cd2", "200 cd7", "8300 cd2"])
def test_hit_synctest_against_the_oracle(name):
    """Every Save's checksum, the final live state and every frame the ring holds."""
    ref = _reference(name)
    g, ids, cks, lists = _gpu_session(name)
    _is_remote_world(g, lists)
    _compare(g, ids, cks, ref, f"hit {name}")
    n, final = SCENARIOS[name][0], ref[1]
    assert (~final["alive"]).sum() > 20 and final["present2"].any() and final["present3"][np.arange(n) % 4 != 0].any()      # entities died; Stun and new Shields exist
    assert (final["c3w0"][final["present3"] & (np.arange(n) % 4 != 0)] == 0xABCD00000007).all()                            # a remotely inserted Shield holds the registered default, an 8-byte word
    if n > 8192:
        links, i = strike_links(n), np.arange(n)
        assert ((links < n) & ((links >> np.uint64(13)) != (i >> 13).astype(np.uint64))).any()      # a sender in one 8192-slot layout tile, its target in the other
        assert final["present2"][8192:].any() and final["present2"][:8192].any() and (~final["alive"][8192:]).any()


def test_p2p_shaped_lists_a_rollback_of_3_then_a_rollback_of_1():
    ref = _reference("p2p")
    g, ids, cks, lists = _gpu_session("p2p")
    assert len(lists) == len(p2p_lists()) and max(sum(isinstance(r, bg.AdvanceFrame) for r in reqs) for reqs in lists) == 4
    _is_remote_world(g, lists)
    _compare(g, ids, cks, ref, "hit p2p")


def test_host_decided_spawns_children_are_not_hit_in_the_frame_they_appear():
    """Every fourth frame five children (a user-written spawn system, host-decided counts); every tenth link points at n + 5 -- the first child of the SECOND batch: the
    commands sent to it in the frame it appears are dropped (the oracle session counted them), from the next frame on they land."""
    ref = _reference("spawn")
    g, ids, cks, lists = _gpu_session("spawn")
    _is_remote_world(g, lists)
    _compare(g, ids, cks, ref, "hit with spawns")
    n = SCENARIOS["spawn"][0]
    assert ref[1]["len"] >= n + 10 and oracle_session("spawn")[4].spawned_this_frame >= 1


def test_a_peer_reading_watcher_registered_first():
    ref = _reference("watcher")
    g, ids, cks, lists = _gpu_session("watcher")
    _is_remote_world(g, lists, peers=True)
    _compare(g, ids, cks, ref, "hit with a watcher")
    seen = ref[1]["c4w0"][ref[1]["alive"]]
    assert (seen % 100 != 0).any() and (seen >= 100).any()                   # the watcher saw stunned targets (1 + ticks) and targets it could not see (100)


def test_specialised_copies_forced_at_first_sight(monkeypatch):
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    ref = _reference("200 cd2")
    g, ids, cks, lists = _gpu_session("200 cd2", before=lambda w: w._lib.ggrs_dbg_set_spec_shapes(w._p, 3))
    assert g.kernel_info()["specialised_kernel"].startswith("ready"), g.kernel_info()["specialised_kernel"]
    _is_remote_world(g, lists)
    _compare(g, ids, cks, ref, "specialised copies")


def test_one_launch_more_per_frame_than_the_same_world_without_remote_bindings():
    """[Save(f), Advance] lists, one frame each: the remote world's frame is the group's launch plus ONE apply."""
    counts = {}
    frames = 6
    for remote in (True, False):
        g, ids = _gpu_world("200 cd2", remote=remote)
        g.set_synctest_check_distance(-1)
        g.handle_requests([bg.SaveGameState(0), bg.AdvanceFrame((1,))])          # (the first list: whatever a first launch does besides)
        g.host_timeline(1)
        for f in range(1, 1 + frames): g.handle_requests([bg.SaveGameState(f), bg.AdvanceFrame((f % 3,))])
        counts[remote] = g.host_timeline(0)["launches"]
        if remote: assert _applies(g)[0] == frames + 1 and not _inbox(g).any()
    assert counts[True] == counts[False] + frames and counts[False] >= frames, counts


def _raw_ring(g, ids):
    """Every frame the ring holds, newest first: the masks and EVERY word of every column below len as the block holds them -- dead and absent slots too."""
    out = {}
    for f in reversed([f for f in range(g.frame + 1) if g.has_snapshot(f)]):
        g.load(f)
        n = g.len
        rec = [g.alive_mask(n).tobytes()]
        for c in ids:
            rec.append(g.present_mask(c, n).tobytes())
            for k in range(g._comps[c][2]): rec.append(g.download_word(c, k, 0, n).tobytes())
        out[f] = b"".join(rec)
    return out


def test_the_same_list_twice_on_fresh_worlds_gives_identical_ring_bytes():
    runs = []
    for _ in range(2):
        g, ids, cks, lists = _gpu_session("200 cd7")
        runs.append((cks, _raw_ring(g, ids)))
    (ca, ra), (cb, rb) = runs
    assert ca == cb and sorted(ra) == sorted(rb) and len(ra) >= 7
    for f in ra: assert ra[f] == rb[f], f"determinism: ring frame {f}"


def _fanout_rank(rank, size, id_q, q):
    """One rank of ggrs_hip_fanout_step's request-list form on the hit world: every rank holds the same world and walks the same two branches."""
    try:
        from bevy_ggrs_amd.fanout import RcclFanout
        if rank == 0:
            id_bytes = RcclFanout.unique_id()
            for _ in range(size - 1): id_q.put(id_bytes)
        else:
            id_bytes = id_q.get(timeout=120)
        n = 200
        g = bg.World(n + 128, max_depth=6, device=0)
        ids = build_hit(g); spawn_hit(g, ids, n); g.set_depth(6)
        native = RcclFanout(g, rank, size, id_bytes)
        reqs = [bg.SaveGameState(0)]
        for b in range(2):
            reqs += [bg.LoadGameState(0), bg.AdvanceFrame((b + 1,)), bg.SaveGameState(1), bg.AdvanceFrame((b + 1,)), bg.SaveGameState(2)]
        ns = native.step(reqs)
        table = native.collect()
        got = [int(p[0]) | (int(p[1]) << 64) for p in np.asarray(table).reshape(-1, 2)]
        g._lib.ggrs_dbg_remote_inbox.restype = C.c_int64
        g._lib.ggrs_dbg_remote_inbox.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        buf = np.full(1 << 12, 0xA5A5A5A5, dtype=np.uint32)
        nb = g._lib.ggrs_dbg_remote_inbox(g._p, buf.ctypes.data, buf.nbytes)
        clean = nb > 0 and not buf[:nb // 4].any()
        native.close()
        q.put((rank, "ok", ns, got, clean))
    except Exception as e:                                    # noqa: BLE001
        import traceback
        q.put((rank, "error", f"{type(e).__name__}: {e}", traceback.format_exc()))


def test_fanout_step_with_two_ranks_on_one_gpu_gives_equal_checksums_on_both_ranks():
    import multiprocessing as mp
    from test_gpu_zfanout import _double_lib                                                   # (a name only: no test is imported)
    ctx = mp.get_context("spawn")
    q, id_q = ctx.Queue(), ctx.Queue()
    old = os.environ.get("GGRS_RCCL_LIB")
    os.environ["GGRS_RCCL_LIB"] = _double_lib()
    try:
        procs = [ctx.Process(target=_fanout_rank, args=(r, 2, id_q, q)) for r in range(2)]
        for p in procs: p.start()
    finally:
        if old is None: os.environ.pop("GGRS_RCCL_LIB", None)
        else: os.environ["GGRS_RCCL_LIB"] = old
    res = {}
    try:
        for _ in range(2):
            r = q.get(timeout=240); res[r[0]] = r[1:]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive(): p.kill()
    for r in (0, 1): assert res[r][0] == "ok" and res[r][1] == 5 and res[r][3], res[r]
    # the oracle's walk of the same list
    o = OracleWorld(200 + 128, 6, FLAT); ido = build_hit(o); spawn_hit(o, ido, 200); o.set_depth(6)
    want = []
    reqs = [bg.SaveGameState(0)]
    for b in range(2): reqs += [bg.LoadGameState(0), bg.AdvanceFrame((b + 1,)), bg.SaveGameState(1), bg.AdvanceFrame((b + 1,)), bg.SaveGameState(2)]
    for rq in reqs: want += o.handle_requests([rq])
    t0, t1 = res[0][2], res[1][2]
    assert t0 == t1 and len(t0) == 2 * 5, (len(t0), len(t1))                 # every rank judges the same gathered table ...
    assert t0[:5] == t0[5:] == want, (t0, want)                              # ... whose two ranks' checksums are equal, and the oracle's
    assert len(set(want[1:])) == 4                                           # (the branches diverge, and so do their frames)


def _branch_rank(q, lib_path):
    try:
        os.environ["GGRS_RCCL_LIB"] = lib_path
        from bevy_ggrs_amd.fanout import RcclFanout
        n = 200
        g = bg.World(n + 128, max_depth=6)
        ids = build_hit(g); spawn_hit(g, ids, n); g.set_depth(6)
        native = RcclFanout(g, 0, 1, RcclFanout.unique_id())
        pre, keep, _ = g.build_requests([bg.SaveGameState(0)])
        inputs = np.zeros((2, 2, 1), dtype=np.uint8)
        bs = _ffi.BranchStep()
        bs.prefix, bs.n_prefix, bs.n_branches, bs.n_frames, bs.n_inputs, bs.flags = pre, 1, 2, 2, 1, _ffi.BRANCH_SAVE_LAST
        bs.inputs = inputs.ctypes.data
        rc = _ffi.lib.ggrs_hip_fanout_step_branches(native._p, C.byref(bs), None)
        msg = (_ffi.lib.ggrs_hip_fanout_last_error(native._p) or b"").decode()
        native.close()
        q.put(("ok", rc, msg))
    except Exception as e:                                    # noqa: BLE001
        import traceback
        q.put(("error", f"{type(e).__name__}: {e}", traceback.format_exc()))


def test_branch_steps_are_refused_with_a_message():
    import multiprocessing as mp
    from test_gpu_zfanout import _double_lib                                                   # (a name only: no test is imported)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_branch_rank, args=(q, _double_lib())); p.start()
    try: r = q.get(timeout=240)
    finally:
        p.join(timeout=60)
        if p.is_alive(): p.kill()
    assert r[0] == "ok", r
    assert r[1] == bg.GGRS_E_INVALID and "remote bindings" in r[2] and "ggrs_hip_fanout_step_branches" in r[2] and "use ggrs_hip_fanout_step" in r[2], r
