"""Deferred Saves (csrc/host_groups.hpp materialise_slots): in a steady rollback session a request group stores only its FIRST Save; every
later ring slot of the group is defined as the base advanced by the recorded steps and is filled by one launch when somebody needs its bytes.
Whatever an observer can see -- every Checksum(u128), every frame the ring holds, the live world -- must be the CPU oracle's, whether the
slots were deferred or not, across rollbacks of every length, host edits, handed-out pointers and deferral switched on and off mid-session -- and in a
world whose kernel reads per-player inputs and a host-computed per-step constant, which a replay can only have from its record."""
import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
from oracle.binding import FLAT, OracleWorld

pytestmark = pytest.mark.gpu

DEFER_FORCED, DEFER_OFF = 3, 4          # ggrs_dbg_set_lazy_live: 3 = lazy live block and deferred Saves on every eligible list, 4 = by size without deferred Saves


_counts = cm.deferred_counts


def _ring_contents(w, ids, frames):
    """Load every frame the ring holds (newest first: a rollback pops what is newer) and record the whole state."""
    out = {}
    for f in sorted(frames, reverse=True):
        if not w.has_snapshot(f): continue
        w.handle_requests([bg.LoadGameState(f)])
        out[f] = {k: (v.tobytes() if hasattr(v, "tobytes") else v) for k, v in cm.snapshot_state(w, ids).items()}
    return out


def _world(kind, n, max_depth, mode=None, vtags=None, cap=None):
    cap = cap or n
    w = bg.World(cap, max_depth=max_depth) if kind == "lib" else OracleWorld(cap, max_depth, FLAT)
    ids = cm.build_particles(w)
    if kind == "lib":
        if vtags is not None: assert w._lib.ggrs_dbg_set_value_tags(w._p, vtags) == 0
        if mode is not None: assert w._lib.ggrs_dbg_set_lazy_live(w._p, mode) == 0
    vel, ttl = cm.synthetic_particles(n, ttl="despawn")
    cm.spawn_particles(w, ids, n, vel, ttl)
    return w, ids


@pytest.mark.parametrize("n,vtags", [(1_000_000, None), (4_000_000, 1)])
def test_steady_synctest_ring_frames_equal_the_oracle(n, vtags):
    """The headline shape (SyncTest, check distance 7): after the Load streak every tick defers seven of its eight Saves; then every frame the
    ring holds is loaded -- each Load of a deferred frame materialises it -- and compared with the oracle's, as is the live world."""
    D = 7
    res = []
    for kind in ("lib", "oracle"):
        w, ids = _world(kind, n, D + 2, vtags=vtags)
        drv = cm.SyncTestDriver(w, D)
        for _ in range(24): drv.tick((0,))
        if kind == "lib":
            d, m = _counts(w)
            assert d >= 7 * 4 and m == 0, w.kernel_info().get("deferred_saves")
            if vtags: assert w.kernel_info()["value_tags"].startswith("on"), w.kernel_info()["value_tags"]
        live = cm.snapshot_state(w, ids)
        frames = list(range(w.frame - D - 1, w.frame + 1))
        res.append((drv.all_checksums, live, _ring_contents(w, ids, frames)))
        if kind == "lib":
            assert _counts(w)[1] > 0
            w.close()
    assert res[0][0] == res[1][0]
    cm.assert_states_equal(res[0][1], res[1][1], "live")
    assert res[0][2].keys() == res[1][2].keys() and len(res[0][2]) >= D
    for f in res[0][2]: cm.assert_states_equal(res[0][2][f], res[1][2][f], f"ring frame {f}")


def test_p2p_rollbacks_keep_landing_on_deferred_slots():
    """BASELINE config 4's pattern (rollbacks of 0..7 frames) with deferral forced on every eligible group: a rollback shorter or longer than
    the previous one loads a deferred slot, overwrites the base of a chain, or pops it."""
    n = 300_000
    res = []
    for kind in ("lib", "oracle"):
        w, ids = _world(kind, n, 9, mode=DEFER_FORCED)
        drv = cm.P2PShapeDriver(w, max_rollback=8, seed=11)
        for _ in range(48): drv.tick()
        if kind == "lib":
            d, m = _counts(w)
            assert d > 0 and m > 0, w.kernel_info().get("deferred_saves")
        res.append((drv.all_checksums, cm.snapshot_state(w, ids), _ring_contents(w, ids, range(drv.frame - 9, drv.frame + 1))))
        if kind == "lib": w.close()
    assert res[0][0] == res[1][0]
    cm.assert_states_equal(res[0][1], res[1][1], "live")
    for f in res[0][2]: cm.assert_states_equal(res[0][2][f], res[1][2][f], f"ring frame {f}")


def test_host_edits_and_column_pointers_in_a_deferring_session():
    """Uploads, a host-side spawn, a despawn, downloads and a handed-out column pointer between steady ticks that defer their Saves."""
    n, D = 450_000, 5
    cap = n + 64
    st = []
    for kind in ("lib", "oracle"):
        w, ids = _world(kind, n, 9, mode=DEFER_FORCED, cap=cap)
        st.append({"w": w, "ids": ids, "drv": cm.SyncTestDriver(w, D)})

    def ticks(k):
        for s in st:
            for _ in range(k): s["drv"].tick((0,))

    def same(ctx):
        assert st[0]["drv"].all_checksums == st[1]["drv"].all_checksums, ctx
        cm.assert_states_equal(cm.snapshot_state(st[0]["w"], st[0]["ids"]), cm.snapshot_state(st[1]["w"], st[1]["ids"]), ctx)

    ticks(12)
    same("steady")
    for s in st:
        T = s["ids"][0]
        s["w"].upload_word(T, 1, 100, np.arange(5000, dtype=np.uint32))
    ticks(4)
    for s in st:
        vel, ttl = cm.synthetic_particles(16, ttl="throughput", seed=7)
        cm.spawn_particles(s["w"], s["ids"], 16, vel, ttl)
    ticks(4)
    for s in st: s["w"].despawn(17)
    ticks(3)
    same("after host edits")
    st[0]["w"].column_device_ptr(st[0]["ids"][1], 0)                    # (reads only: the oracle has nothing to hand out)
    ticks(4)
    same("after a column pointer")
    d, m = _counts(st[0]["w"])
    assert d > 0 and m > 0, st[0]["w"].kernel_info().get("deferred_saves")
    frames = range(st[0]["w"].frame - D - 1, st[0]["w"].frame + 1)
    rings = [_ring_contents(s["w"], s["ids"], frames) for s in st]
    for f in rings[0]: cm.assert_states_equal(rings[0][f], rings[1][f], f"ring frame {f}")
    st[0]["w"].close()


@pytest.mark.parametrize("n", [100_000, 450_000])
def test_deferral_switched_on_and_off_within_one_session(n):
    """One session, deferral forced on and off every few ticks (at 100 k with depth-parallel roles), against a world that never defers and
    the oracle: checksums and every ring frame identical."""
    D = 7
    res = []
    for kind, mode in (("lib", DEFER_FORCED), ("lib", DEFER_OFF), ("oracle", None)):
        w, ids = _world(kind, n, D + 2, mode=mode)
        drv = cm.SyncTestDriver(w, D)
        for t in range(30):
            if kind == "lib" and mode == DEFER_FORCED: assert w._lib.ggrs_dbg_set_lazy_live(w._p, DEFER_FORCED if (t // 3) % 2 == 0 else DEFER_OFF) == 0
            drv.tick((0,))
        if kind == "lib":
            d = _counts(w)[0]
            assert (d > 0) == (mode == DEFER_FORCED), w.kernel_info().get("deferred_saves")
        res.append((drv.all_checksums, cm.snapshot_state(w, ids), _ring_contents(w, ids, range(w.frame - D - 1, w.frame + 1))))
        if kind == "lib": w.close()
    for r in res[:2]:
        assert r[0] == res[2][0]
        cm.assert_states_equal(r[1], res[2][1], "live")
        assert r[2].keys() == res[2][2].keys()
        for f in r[2]: cm.assert_states_equal(r[2][f], res[2][2][f], f"ring frame {f}")


# ---- a world whose kernel reads what a replay has to get from its record: box_game (inputs per player, FRICTION.powf(dt) in aux_bits) with Player under rollback ----
def _box_world(kind, n, max_depth, players, mode=None):
    from test_box_game import build_box
    w = bg.World(n + 8, max_depth=max_depth) if kind == "lib" else OracleWorld(n + 8, max_depth, FLAT)
    if kind == "lib" and mode is not None: assert w._lib.ggrs_dbg_set_lazy_live(w._p, mode) == 0
    ids, *_ = build_box(w, n, players, seed=3, spread=True, checksums=[(0, [0, 1, 2]), (1, [0, 1, 2])], player_rollback=True)
    return w, ids


def _box_inputs(frame, players, again=0):
    """Four input bits per player, different for every frame and player -- and for every time the frame is advanced again (`again`: a prediction that was corrected)."""
    return tuple(int(x) for x in np.random.default_rng([23, frame, again]).integers(0, 16, players))


def _same(res):
    assert res[0][0] == res[1][0]
    cm.assert_states_equal(res[0][1], res[1][1], "live")
    assert res[0][2].keys() == res[1][2].keys()
    for f in res[0][2]: cm.assert_states_equal(res[0][2][f], res[1][2][f], f"ring frame {f}")


def test_steady_synctest_of_a_world_that_reads_inputs_defers_by_the_natural_rule():
    """No debug hook: box_game above the size where bytes bound a launch, SyncTest with check distance 7, every frame and player its own input bits.  After the Load
    streak the ticks defer on their own; every ring frame loaded afterwards is replayed from the recorded inputs, n_inputs, dt_bits and aux_bits."""
    n, D, players = 450_000, 7, 3
    res = []
    for kind in ("lib", "oracle"):
        w, ids = _box_world(kind, n, D + 2, players)
        drv = cm.SyncTestDriver(w, D, num_players=players)
        for t in range(24): drv.tick(_box_inputs(t, players))
        if kind == "lib":
            assert w.kernel_info()["deferred_saves"].startswith("on"), w.kernel_info()["deferred_saves"]
            d, m = _counts(w)
            assert d >= (D - 1) * 4 and m == 0, w.kernel_info()["deferred_saves"]
        live = cm.snapshot_state(w, ids)
        res.append((drv.all_checksums, live, _ring_contents(w, ids, range(w.frame - D - 1, w.frame + 1))))
        if kind == "lib":
            assert _counts(w)[1] > 0, w.kernel_info()["deferred_saves"]
            w.close()
    _same(res)
    assert len(res[0][2]) >= D


def test_a_corrected_prediction_is_replayed_with_the_bytes_of_its_own_advance():
    """P2P-shaped rollbacks of 0..7 frames, deferral forced: a rollback advances frames AGAIN with input bytes that differ from the first time (the prediction was
    wrong).  The record of a deferring group must hold the inputs of the advance that produced the slot, not of an earlier or later advance of the same frame."""
    n, players = 450_000, 4
    res = []
    for kind in ("lib", "oracle"):
        w, ids = _box_world(kind, n, 9, players, mode=DEFER_FORCED)
        times = {}

        def inputs(frame, times=times):
            times[frame] = times.get(frame, -1) + 1
            return _box_inputs(frame, players, times[frame])
        drv = cm.P2PShapeDriver(w, max_rollback=8, seed=29, inputs=inputs)
        for _ in range(40): drv.tick()
        assert max(times.values()) >= 2                                      # frames were advanced three times and more, each time with other bytes
        if kind == "lib":
            d, m = _counts(w)
            assert d > 0 and m > 0, w.kernel_info()["deferred_saves"]
        res.append((drv.all_checksums, cm.snapshot_state(w, ids), _ring_contents(w, ids, range(drv.frame - 9, drv.frame + 1))))
        if kind == "lib": w.close()
    _same(res)
    assert len(res[0][2]) >= 2


@pytest.mark.parametrize("between", ["confirmed_past_the_base", "depth_shrinks_below_the_chain", "frame_rate_changes"])
def test_confirmation_depth_and_frame_rate_move_between_a_deferring_group_and_the_read(between):
    """One deferring group [Load(1), (Advance, Save) x 4] -- base frame 2; frames 3, 4, 5 owed --, then, before anybody reads an owed slot:
    ConfirmedFrameCount moves past the base (the next Saves prune the base and frame 3 and land in their blocks: the chain is filled from the base before it is
    overwritten), the depth shrinks so that the base leaves the ring while its block still holds the bytes the chain is replayed from, or the frame rate
    changes (the replay must step with the recorded dt_bits and FRICTION.powf(dt), not the world's current ones).  Then what remains is loaded."""
    n, players = 100_000, 2
    S, L, A = bg.SaveGameState, bg.LoadGameState, lambda f, again=0: bg.AdvanceFrame(_box_inputs(f, players, again))
    res = []
    for kind in ("lib", "oracle"):
        w, ids = _box_world(kind, n, 9, players, mode=DEFER_FORCED)
        w.set_depth(8)
        if kind == "lib": w.set_synctest_check_distance(-1)
        cks, ring = [], {}

        def look(f):
            cks.extend(w.handle_requests([L(f)]))
            ring[f] = cm.snapshot_state(w, ids)
        cks += w.handle_requests([S(0), A(0), S(1), A(1), S(2), A(2), S(3), A(3)])
        cks += w.handle_requests([L(1), A(1, 1), S(2), A(2, 1), S(3), A(3, 1), S(4), A(4, 1), S(5)])        # (ends with a Save: the live block is written, nothing reads the chain yet)
        if kind == "lib": assert _counts(w) == (3, 0), w.kernel_info()["deferred_saves"]
        if between == "confirmed_past_the_base":
            w.set_confirmed(4)
            cks += w.handle_requests([A(5), S(6), A(6), S(7)])
            assert [w.has_snapshot(f) for f in range(2, 8)] == [False, False, True, True, True, True]
            look(5); look(4)
        elif between == "depth_shrinks_below_the_chain":
            w.set_depth(3)
            cks += w.handle_requests([A(5), S(6)])
            assert [w.has_snapshot(f) for f in range(2, 7)] == [False, False, True, True, True]
            look(5); look(4)
        else:
            w.set_frame_rate(30)
            look(4); look(3)
            cks += w.handle_requests([A(3, 2), S(4), A(4, 2), S(5)])
            look(5); look(2)
        if kind == "lib": assert _counts(w)[1] > 0, w.kernel_info()["deferred_saves"]
        cks += w.handle_requests([A(9), S(w.frame + 1), A(10), S(w.frame + 2)])
        res.append((cks, cm.snapshot_state(w, ids), ring))
        if kind == "lib": w.close()
    _same(res)
