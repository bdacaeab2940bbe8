"""ggrs_hip_fanout_step_branches / ggrs_hip_fanout_adopt on worlds with live-only state: a system that can call despawn_rollback() (RollbackDespawned markers,
src/snapshot/despawn.rs:114-143), a non-rollback component, a host-issued marker.  Everything is compared bit for bit with the oracle walking the same branches
as request lists ([Load(F), (Advance, Save) x T] per branch, then Load(F)); observed with `state()` of tests/test_despawn_rollback.py: columns, masks, `disabled`,
`dframe`.  The world is tests/branch_marks_common.py's: odd slots defer their despawn, even slots are freed at once and lose their `Mesh`.

Each test runs in a child process of its own (one RCCL communicator per world; world size 1 over the real RCCL, two ranks over the transport double)."""
import multiprocessing as mp
import os

import pytest

pytestmark = pytest.mark.gpu


def _setup(n, cap, depth=8):
    import bevy_ggrs_amd as bg
    import branch_marks_common as bm
    from bevy_ggrs_amd.fanout import RcclFanout
    from oracle.binding import FLAT, OracleWorld
    gw, ow = bg.World(cap, max_depth=depth), OracleWorld(cap, depth, FLAT)
    ids = None
    for w in (gw, ow):
        ids = bm.build_health(w, n)
        w.set_depth(depth)
        w.set_confirmed(0)
    return gw, ow, ids, RcclFanout(gw, 0, 1, RcclFanout.unique_id())


def _compare(gw, ow, ids, ctx):
    import common as cm
    from test_despawn_rollback import state
    assert gw.frame == ow.frame and gw.len == ow.len, (ctx, gw.frame, ow.frame, gw.len, ow.len)
    cm.assert_states_equal(state(gw, ids), state(ow, ids), str(ctx))


def _case_first(n, cap, Bs, T, preds=None):
    """prefix [Save(0)] under ConfirmedFrameCount 0: every frame of a branch is unconfirmed."""
    import numpy as np
    import bevy_ggrs_amd as bg
    import branch_marks_common as bm
    from bevy_ggrs_amd import _ffi
    from test_despawn_rollback import state
    out = []
    for B in Bs:
        for save_last in (True, False) if preds is None else (True,):
            gw, ow, ids, native = _setup(n, cap)
            pred = np.array(preds, dtype=np.uint8) if preds is not None else np.random.default_rng([n, B, T]).integers(0, 3, size=(B, T)).astype(np.uint8)
            prefix = [bg.SaveGameState(0)]
            want = bm.oracle_walk(ow, prefix, 0, pred, save_last)
            rc, got = bm.library_step(native, gw, prefix, pred, _ffi.BRANCH_SAVE_LAST if save_last else 0)
            assert rc == 0, (B, save_last, rc, got)
            assert got[0] == want, (B, save_last, "the branch table")
            assert gw.frame == 0
            _compare(gw, ow, ids, (n, B, save_last))
            s = state(ow, ids)
            out.append((int(s["present1"].sum()), int(s["disabled"].sum())))
            native.close()
    return out


def _case_live_markers(n, cap):
    """Two AdvanceFrames while ConfirmedFrameCount lags leave markers in the live world; then it moves, so a DespawnConfirmed is pending when the branches start."""
    import numpy as np
    import bevy_ggrs_amd as bg
    import branch_marks_common as bm
    from bevy_ggrs_amd import _ffi
    from test_despawn_rollback import state
    out = []
    for confirmed in (1, 2):                                     # frame 1's markers, then frame 2's too, are confirmed before the members start
        gw, ow, ids, native = _setup(n, cap)
        for w in (gw, ow):
            w.handle_requests([bg.AdvanceFrame((1,)), bg.AdvanceFrame((1,))])
        before = state(ow, ids)
        assert before["disabled"].sum() > 0 and set(before["dframe"][before["disabled"]]) == {1, 2}
        _compare(gw, ow, ids, "before")
        for w in (gw, ow): w.set_confirmed(confirmed)
        pred = np.array([[1, 0, 1], [0, 2, 0], [2, 1, 0], [0, 0, 0]], dtype=np.uint8)
        prefix = [bg.SaveGameState(2)]
        want = bm.oracle_walk(ow, prefix, 2, pred, True)
        rc, got = bm.library_step(native, gw, prefix, pred, _ffi.BRANCH_SAVE_LAST)
        assert rc == 0, (confirmed, rc, got)
        assert got[0] == want, (confirmed, "the branch table")
        _compare(gw, ow, ids, ("after", confirmed))
        after = state(ow, ids)
        out.append((int(before["disabled"].sum()), int(after["disabled"].sum())))
        native.close()
    return out


def _case_adopt(n, cap, retain_all, k, T=4, B=5):
    """Three branch steps in a row (the later ones behind a prefix that advances), then the adoption of a retained branch and one more tick.

    The earlier steps leave their records' words behind, so the adoption reads the last step's or fails.  What this cannot show is a LATER step with a SMALLER cover
    than an earlier one: a retained step's cover is at least the mask extent (`dirty_len`) of every block it retains into, those blocks are reused from step to step
    and an extent never shrinks, so while records exist the cover only grows -- `BranchKeep::units` bounds the reads by the launch that wrote them all the same."""
    import numpy as np
    import bevy_ggrs_amd as bg
    import branch_marks_common as bm
    from bevy_ggrs_amd import _ffi
    from test_despawn_rollback import state
    gw, ow, ids, native = _setup(n, cap, depth=10)
    rng = np.random.default_rng([n, int(retain_all), k])
    flags = _ffi.BRANCH_SAVE_LAST | (_ffi.BRANCH_RETAIN_ALL if retain_all else _ffi.BRANCH_RETAIN_NEWEST)
    F = pred = None
    for step in range(3):
        Cf = gw.frame
        for w in (gw, ow): w.set_confirmed(Cf)                    # ConfirmedFrameCount moves between the steps: the prefix's AdvanceFrame frees what it confirms
        if step == 0: prefix, F = [bg.SaveGameState(Cf)], Cf
        else: prefix, F = [bg.LoadGameState(Cf), bg.AdvanceFrame((int(rng.integers(0, 2)),)), bg.SaveGameState(Cf + 1)], Cf + 1
        pred = rng.integers(0, 2, size=(B, T)).astype(np.uint8)       # (every step of a fan-out has the agreed shape; the records of the earlier steps stay behind, stale)
        want = bm.oracle_walk(ow, prefix, F, pred, True)
        rc, got = bm.library_step(native, gw, prefix, pred, flags)
        assert rc == 0, (step, rc, got)
        assert got[0] == want, (step, "the branch table")
        _compare(gw, ow, ids, ("step", step))
    b = int(rng.integers(0, pred.shape[0]))
    native.adopt(b, F + k)
    ow.handle_requests(bm.branch_requests(F, pred[b], k, True, T, saves=False))
    _compare(gw, ow, ids, ("adopted", b, k))
    adopted = state(ow, ids)
    assert gw.save() == ow.save(), "SaveGameState after the adoption"
    for w in (gw, ow): w.set_confirmed(w.frame)
    tick = [bg.SaveGameState(F + k), bg.AdvanceFrame((0,)), bg.SaveGameState(F + k + 1)]
    assert list(gw.handle_requests(tick)) == list(ow.handle_requests(tick)), "the tick after the adoption"
    _compare(gw, ow, ids, "the tick after the adoption")
    assert not state(gw, ids)["disabled"].any(), "the adopted markers are confirmed: the next AdvanceFrame frees them"
    native.close()
    return int(adopted["disabled"].sum())


def _case_host_marker(n):
    """The particles world: no system can defer, the kernel has no marker text; a host-issued despawn_rollback() on an unconfirmed frame leaves markers the branch step
    must neither read nor touch."""
    import numpy as np
    import bevy_ggrs_amd as bg
    import common as cm
    import branch_marks_common as bm
    from bevy_ggrs_amd import _ffi
    from bevy_ggrs_amd.fanout import RcclFanout
    from oracle.binding import FLAT, OracleWorld
    from test_despawn_rollback import state
    gw, ow = bg.World(n + 64, max_depth=8), OracleWorld(n + 64, 8, FLAT)
    for w in (gw, ow):
        ids = cm.build_particles(w)
        vel, ttl = cm.synthetic_particles(n, ttl="despawn")
        cm.spawn_particles(w, ids, n, vel, ttl)
        w.set_depth(8); w.set_confirmed(0)
        w.handle_requests([bg.AdvanceFrame((0,)), bg.AdvanceFrame((0,))])
        for slot in range(40, 46): w.despawn_rollback(slot)      # frame 2 is unconfirmed: disabled, not freed
    native = RcclFanout(gw, 0, 1, RcclFanout.unique_id())
    pred = np.zeros((5, 3), dtype=np.uint8)
    prefix = [bg.SaveGameState(2)]
    want = bm.oracle_walk(ow, prefix, 2, pred, True)
    rc, got = bm.library_step(native, gw, prefix, pred, _ffi.BRANCH_SAVE_LAST)
    assert rc == 0, (rc, got)
    assert got[0] == want, "the branch table"
    _compare(gw, ow, ids, "after")
    s = state(gw, ids)
    native.close()
    return s["disabled"][40:46].tolist(), s["dframe"][40:46].tolist(), int(s["disabled"].sum())


def _child(q, fn, args):
    try:
        q.put(("ok", globals()[fn](*args)))
    except Exception as e:                                    # noqa: BLE001 -- reported to the parent
        import traceback
        q.put(("error", f"{type(e).__name__}: {e}", traceback.format_exc()))


def _run(fn, *args, timeout=240):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(q, fn, args)); p.start()
    try: r = q.get(timeout=timeout)
    finally:
        p.join(timeout=30)
        if p.is_alive(): p.kill()
    assert r[0] == "ok", r
    return r[1]


def test_branch_step_of_a_marker_world_matches_the_list_walk():
    """300 entities in a capacity-400 world (5 units, the last one partial, 2 workgroups), 3 branches x 2 frames.  The parent commit refuses this world with
    GGRS_E_INVALID.  Afterwards the world stands at frame 0 as the oracle's does after its closing Load(0): 210 entities still have their Mesh, no marker is left."""
    assert _run("_case_first", 300, 400, [3], 2, [[1, 1], [2, 0], [0, 3]]) == [(210, 0)]


@pytest.mark.parametrize("B", [1, 5, 17])
def test_branch_step_past_one_round_of_workgroups(B):
    """2 300 entities: 9 workgroups, past one round of the 8-XCD tile mapping; 4 frames, with and without GGRS_BRANCH_SAVE_LAST."""
    assert len(_run("_case_first", 2300, 2400, [B], 4)) == 2


def test_markers_already_in_the_live_world_and_a_pending_despawn_confirmed():
    res = _run("_case_live_markers", 300, 400)
    assert len(res) == 2 and res[0][1] < res[0][0] and res[1][1] == 0, res       # ConfirmedFrameCount 1 frees frame 1's markers before the members start


@pytest.mark.parametrize("retain_all,k", [(True, 2), (True, 4), (False, 4)])
def test_adoption_of_a_retained_branch_merges_its_markers(retain_all, k):
    assert _run("_case_adopt", 1500, 1600, retain_all, k) > 0, "the adopted branch deferred nothing: the test checks nothing"


def test_a_host_issued_marker_is_left_alone():
    dis, df, total = _run("_case_host_marker", 3000)
    assert dis == [True] * 6 and df == [2] * 6 and total == 6


# ---- two ranks over the transport double
def _rank(rank, size, id_q, q, mode):
    try:
        import numpy as np
        import bevy_ggrs_amd as bg
        import branch_marks_common as bm
        import common as cm
        from bevy_ggrs_amd import _ffi
        from bevy_ggrs_amd.fanout import RcclFanout
        from oracle.binding import FLAT, OracleWorld
        from test_despawn_rollback import state
        if rank == 0:
            id_bytes = RcclFanout.unique_id()
            for _ in range(size - 1): id_q.put(id_bytes)
        else:
            id_bytes = id_q.get(timeout=120)
        n, cap, T, bpr = 600, 700, 3, 3
        gw, ow = bg.World(cap, max_depth=8), OracleWorld(cap, 8, FLAT)
        for w in (gw, ow):
            ids = bm.build_health(w, n)                              # the same world on every rank (the live-only side is not part of a state broadcast)
            w.set_depth(8); w.set_confirmed(0)
        native = RcclFanout(gw, rank, size, id_bytes)
        base = np.array([[1, 1, 0], [0, 2, 1], [2, 0, 0]], dtype=np.uint8)
        preds = [np.roll(base, r, axis=0) for r in range(size)]      # every rank walks the same branches in another order: the same entities lose their Mesh everywhere
        prefix = [bg.SaveGameState(0)]
        want = []
        for r in range(size):
            if r == rank: want.append(bm.oracle_walk(ow, prefix, 0, preds[r], True))
            else:
                o2 = OracleWorld(cap, 8, FLAT); bm.build_health(o2, n); o2.set_depth(8); o2.set_confirmed(0)
                want.append(bm.oracle_walk(o2, prefix, 0, preds[r], True))
        rc, got = bm.library_step(native, gw, prefix, preds[rank], _ffi.BRANCH_SAVE_LAST | _ffi.BRANCH_RETAIN_ALL)
        assert rc == 0, (rc, got)
        assert got == want, "the gathered table"
        cm.assert_states_equal(state(gw, ids), state(ow, ids), "after the step")
        owner, local, k = 1, 1, T
        row = preds[owner][local]
        replay = None
        if mode == _ffi.ADOPT_RECOMPUTE and rank != owner: replay = bm.branch_requests(0, row, k, True, T, saves=False, final_save=True)
        native.adopt(owner * bpr + local, k, replay, mode)
        ow.handle_requests(bm.branch_requests(0, row, k, True, T, saves=False, final_save=True))
        assert gw.frame == ow.frame == k
        s_adopted = state(gw, ids)
        cm.assert_states_equal(s_adopted, state(ow, ids), "adopted")
        for w in (gw, ow): w.set_confirmed(w.frame)
        tick = [bg.SaveGameState(k), bg.AdvanceFrame((1,)), bg.SaveGameState(k + 1)]
        cs = list(gw.handle_requests(tick))
        assert cs == list(ow.handle_requests(tick)), "the tick after the adoption"
        s_tick = state(gw, ids)
        cm.assert_states_equal(s_tick, state(ow, ids), "the tick after the adoption")
        native.close()
        plain = lambda s: {k_: (v.tolist() if hasattr(v, "tolist") else v) for k_, v in s.items()}
        q.put((rank, "ok", plain(s_adopted), plain(s_tick), cs))
    except Exception as e:                                    # noqa: BLE001 -- reported to the parent
        import traceback
        q.put((rank, "error", f"{type(e).__name__}: {e}", traceback.format_exc()))


@pytest.mark.parametrize("mode", ["recompute", "broadcast"])
def test_two_ranks_adopt_a_marker_branch(mode):
    from bevy_ggrs_amd import _ffi
    from test_gpu_zfanout import _double_lib
    ctx = mp.get_context("spawn")
    q, id_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, 2, id_q, q, _ffi.ADOPT_BROADCAST if mode == "broadcast" else _ffi.ADOPT_RECOMPUTE)) for r in range(2)]
    old = os.environ.get("GGRS_RCCL_LIB")
    os.environ["GGRS_RCCL_LIB"] = _double_lib()               # spawned children inherit the parent's environment at start()
    try:
        for p in procs: p.start()
    finally:
        if old is None: os.environ.pop("GGRS_RCCL_LIB", None)
        else: os.environ["GGRS_RCCL_LIB"] = old
    res = {}
    try:
        for _ in range(2):
            r = q.get(timeout=240)
            res[r[0]] = r[1:]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive(): p.kill()
    assert all(res[r][0] == "ok" for r in (0, 1)), res
    assert res[0][1:] == res[1][1:], "the ranks differ"
    assert sum(res[0][1]["disabled"]) > 0, "the adopted branch deferred nothing: the test checks nothing"
