"""Device-resident rollback resources (ggrs_hip_register_resource / _add_resource_system / _add_custom_system_resources): a world-global value that evolves once per
frame inside the generated kernel -- every wave carries it in scalar registers and replays the resource systems itself -- so that a rollback restores and replays it.
Everything goes through the C ABI and is bit-exact: the Checksum(u128) of every SaveGameState equals the CPU oracle's XOR the resource parts of the Python model kept
beside it (resources_common.ClockModel; the oracle has no resources), the final state and every frame the ring holds equal the oracle's, and resource_read of every
resource equals the model's value at that frame.

Shapes: 130 slots (two full waves and a 2-lane tail), 300 (crosses the 256-slot workgroup), 8262 (crosses the 8192-slot layout tile; 12 ticks at check distance 2:
the oracle calls Python once per entity, system and frame), 1 048 646 for the in-place test (4097 workgroups, twice what the device holds at once; built-in systems
only on the oracle side).  An oracle session is computed once per shape and shared, unchanged, by the tests that compare against it."""
import ctypes as C
import functools

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
import resources_common as rc
from bevy_ggrs_amd import _ffi
from oracle.binding import FLAT, OracleWorld

pytestmark = pytest.mark.gpu
DEPTH = 8
U32 = np.uint32


def _setup(w, n, model=None, **kw):
    ids = rc.build_clock(w, **({"model": model} if isinstance(w, OracleWorld) else {}), **kw)
    rc.spawn_clock(w, ids, n)
    w.set_depth(DEPTH)
    return ids


def _ring_states(w, ids, resources=False):
    """Every frame the ring holds, loaded newest first (a Load pops the newer snapshots): the state and -- a library world -- the resources the Load restored."""
    out = {}
    for f in reversed([f for f in range(w.frame + 1) if w.has_snapshot(f)]):
        w.load(f)
        out[f] = (cm.snapshot_state(w, ids), rc.read_resources(w) if resources else None)
    return out


@functools.lru_cache(maxsize=None)
def _reference(n, cd, ticks):
    """The oracle's session with the model beside it: ([(frame, checksum ^ resource parts)], final state, {frame: state} of the ring, the model)."""
    o = OracleWorld(n + 128, DEPTH, FLAT)
    model = rc.ClockModel()
    ids = _setup(o, n, model)
    got = []
    for reqs in rc.synctest_lists(cd, ticks, DEPTH): rc.run_model(o, model, reqs, cd=cd, got=got)
    final = cm.snapshot_state(o, ids)
    assert 0 < int(final["alive"].sum()) < n, "entities die mid-session, not all of them"
    cur = list(model.cur)
    return got, final, {f: s for f, (s, _) in _ring_states(o, ids).items()}, model, cur


def _gpu_session(n, cd, ticks, *, before=None, cap=None):
    g = bg.World(cap or n + 128, max_depth=DEPTH)
    if before: before(g)
    ids = _setup(g, n)
    g.set_synctest_check_distance(cd)
    lists = rc.synctest_lists(cd, ticks, DEPTH)
    cks = []
    for reqs in lists: cks += g.handle_requests(reqs)
    frames = [r.frame for reqs in lists for r in reqs if isinstance(r, bg.SaveGameState)]
    return g, ids, list(zip(frames, cks))


def _compare(g, ids, cks, ref, ctx, cd):
    want, final, ring_states, model, cur = ref
    assert len(cks) == len(want) > 0, (len(cks), len(want))
    for (fa, ca), (fb, cb) in zip(cks, want):
        assert fa == fb and ca == cb, f"{ctx}: frame {fa}: gpu {ca:#x} oracle ^ model {cb:#x}"
    cm.assert_states_equal(cm.snapshot_state(g, ids), final, ctx)
    assert rc.read_resources(g) == model.words(cur), (ctx, rc.read_resources(g), model.words(cur))
    got = _ring_states(g, ids, resources=True)
    assert sorted(got) == sorted(ring_states) and len(got) >= min(cd, 2), (sorted(got), sorted(ring_states))
    for f, (state, res) in got.items():
        cm.assert_states_equal(state, ring_states[f], f"{ctx}: ring frame {f}")
        assert res == model.words(model.snaps[f]), (ctx, f, res, model.words(model.snaps[f]))


def _is_resource_world(g):
    """Every policy stays on for such a world: nothing was switched off to make it pass."""
    info = g.kernel_info()
    assert info["request_group_kernel"].startswith("ggrs_jit_tick"), info
    assert "live-only state" not in info["lazy_live_block"] and info["deferred_saves"].startswith("on"), info
    assert not info["group_caps"].endswith("/ 1 steps") and info["device_resources"].startswith("3 resources, 20 bytes"), info


@pytest.mark.parametrize("n,cd,ticks", [(130, 2, 40), (130, 7, 24), (300, 2, 40), (300, 7, 24), (8262, 2, 12)])
def test_clock_synctest_against_the_oracle_and_the_model(n, cd, ticks):
    ref = _reference(n, cd, ticks)
    g, ids, cks = _gpu_session(n, cd, ticks)
    _is_resource_world(g)
    _compare(g, ids, cks, ref, f"clock {n} cd {cd}", cd)
    # registering after seal is refused
    with pytest.raises(bg.GgrsHipError) as e: g.register_resource("Late", 4, 1)
    assert e.value.code == bg.GGRS_E_INVALID and "'Late'" in str(e.value) and "sealed" in str(e.value)
    with pytest.raises(bg.GgrsHipError) as e: g.add_resource_system(rc.TICK_SRC, [(0, 0), (0, 1), (1, 0), (2, 0)], name="late")
    assert e.value.code == bg.GGRS_E_INVALID and "'late'" in str(e.value) and "sealed" in str(e.value)


def test_p2p_shaped_rollbacks_whose_inputs_change_between_prediction_and_confirmation():
    """Rollbacks of 0 to 7 frames; a re-simulated frame sees another input than its first simulation, so the seed chain differs: a wrong restore shows."""
    n = 300
    lists = rc.p2p_lists(36)
    assert {sum(isinstance(r, bg.LoadGameState) for r in reqs) for _, reqs in lists} == {0, 1}
    assert {len([r for r in reqs if isinstance(r, bg.AdvanceFrame)]) - 1 for _, reqs in lists} == set(range(8))
    o = OracleWorld(n + 128, DEPTH, FLAT); model = rc.ClockModel(); ido = _setup(o, n, model)
    g = bg.World(n + 128, max_depth=DEPTH); ids = _setup(g, n)
    g.set_synctest_check_distance(-1)
    want, got = [], []
    for confirmed, reqs in lists:
        rc.run_model(o, model, reqs, confirmed=confirmed, got=want)
        if confirmed is not None: g.set_confirmed(confirmed)
        cs = g.handle_requests(reqs)
        got += list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], cs))
    assert got == want and len(got) > 100
    cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), "p2p-shaped lists")
    assert rc.read_resources(g) == model.words()
    rg, ro = _ring_states(g, ids, resources=True), _ring_states(o, ido)
    assert sorted(rg) == sorted(ro) and len(rg) >= 7
    for f in rg:
        cm.assert_states_equal(rg[f][0], ro[f][0], f"p2p ring frame {f}")
        assert rg[f][1] == model.words(model.snaps[f]), f


def test_order_a_system_registered_before_tick_sees_the_old_value_one_after_it_the_new():
    g = bg.World(256, max_depth=DEPTH); ids = _setup(g, 70, fuse_step=0); P, S, Fz = ids
    g.resource_write(0, [41, 7])                                                                 # a known state
    g.handle_requests([bg.SaveGameState(0), bg.AdvanceFrame((5,), dt_bits=rc.DT_BITS)])
    assert set(g.download_word(S, 0, 0, 70).tolist()) == {41} and set(g.download_word(S, 1, 0, 70).tolist()) == {42}
    m = rc.ClockModel(); m.cur[0], m.cur[1] = 41, 7; m.step(5)
    assert rc.read_resources(g) == m.words()
    x0 = ((np.arange(70) % 17) * 0.25 - 1.0).astype(np.float32)
    want = (x0 + np.float32(rc.bits_f32(m.cur[2]) * rc.DT)).astype(np.float32)
    assert (g.download_word(P, 0, 0, 70).view(np.float32) == want).all()


def _big_lists():
    """Plain ticks (live -> live, no Load) and lists in which a Save lands on the slot the group loaded: Load(F) pops F's slot, Save(F) takes it back."""
    a = lambda f: bg.AdvanceFrame(((f * 3 + 1) & 15,), dt_bits=rc.DT_BITS)      # noqa: E731
    return [[bg.SaveGameState(0), a(0)], [bg.SaveGameState(1), a(1)], [bg.SaveGameState(2), a(2)],
            [bg.LoadGameState(2), bg.SaveGameState(2), a(2), bg.SaveGameState(3), a(3)],
            [bg.SaveGameState(4), a(4)], [bg.LoadGameState(4), bg.SaveGameState(4), a(4)], [bg.SaveGameState(5), a(5)]]


def test_in_place_launches_at_4097_workgroups():
    """No launch may read resource words from a location it writes: live -> live and a Save into the slot the group loaded, with a grid of 4097 workgroups -- half of
    it is dispatched after workgroup 0 has stored."""
    n = 1_048_646
    o = OracleWorld(n + 64, 4, FLAT); model = rc.ClockModel(); ido = rc.build_big(o)
    g = bg.World(n + 64, max_depth=4); ids = rc.build_big(g)
    init = (np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(U32)
    for w, wi in ((o, ido), (g, ids)): w.spawn(n, {wi[0]: [init]}); w.set_depth(4)
    g.set_synctest_check_distance(-1)
    for k, reqs in enumerate(_big_lists()):
        want = rc.run_model(o, model, reqs)
        cs = g.handle_requests(reqs)
        got = list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], cs))
        assert got == want, (k, got, want)
        assert rc.read_resources(g) == model.words(), (k, rc.read_resources(g), model.words())
    assert (g.download_word(ids[0], 0, n - 5, 5) == o.download_word(ido[0], 0, n - 5, 5)).all() and g.frame == 6
    for f in (5, 4):
        g.load(f)
        assert rc.read_resources(g) == model.words(model.snaps[f]), f


def _many(w, extra):
    """`extra` entities that have Fuse alone: no user-written system visits them (the oracle stays cheap), the launch covers them."""
    if extra: w.spawn(extra, {2: [np.full(extra, 1 << 20, dtype=U32)]})


def _route_session(cap, extra, how):
    g = bg.World(cap, max_depth=DEPTH); ids = _setup(g, 300); _many(g, extra)
    g.set_synctest_check_distance(2)
    cks, inflight = [], 0
    for reqs in rc.synctest_lists(2, 14, DEPTH):
        if how == "blocking": cks += g.handle_requests(reqs); continue
        g.enqueue_requests(reqs); inflight += 1                                  # two lists in flight: the next launch on the stream folds the previous one's rows
        if inflight == 2: cks += g.collect_checksums(); inflight -= 1
    while inflight: cks += g.collect_checksums(); inflight -= 1
    return g, cks


def test_every_fold_route_gives_the_same_checksums():
    """The host's fold, fold-forward (enqueue / collect above 1024 workgroups) and self-fold (blocking calls there); k_gen_finalize and its device copy run in the
    fan-out test below.  The same session, so the same u128s; the oracle + model for the large world (most of its entities have Fuse alone)."""
    extra = 270_000
    o = OracleWorld(300 + extra + 128, DEPTH, FLAT); model = rc.ClockModel(); _setup(o, 300, model); _many(o, extra)
    want = []
    for reqs in rc.synctest_lists(2, 14, DEPTH): rc.run_model(o, model, reqs, cd=2, got=want)
    want = [c for _, c in want]
    g_ff, ff = _route_session(300 + extra + 128, extra, "enqueue")
    g_sf, sf = _route_session(300 + extra + 128, extra, "blocking")
    assert g_ff.kernel_info()["checksum_fold"].startswith("fold-forward") and "self-fold" in g_sf.kernel_info()["checksum_fold"], g_ff.kernel_info()["checksum_fold"]
    assert ff == want and sf == want
    # the host folds: the small world, whose Fuse-only entities are absent -- against ITS reference, and the routes agree on the resource part (oracle parts differ by the extra entities only)
    g_h, hf = _route_session(428, 0, "blocking")
    assert g_h.kernel_info()["checksum_fold"].startswith("the host folds the rows"), g_h.kernel_info()["checksum_fold"]
    assert hf == [c for _, c in _reference(300, 2, 40)[0]][:len(hf)]
    g_he, he = _route_session(428, 0, "enqueue")
    assert he == hf


def _lazy(w): w._lib.ggrs_dbg_set_lazy_live(w._p, 3)


def test_knob_every_group_defers_its_saves_and_leaves_the_live_block():
    n, cd, ticks = 300, 2, 40
    g, ids, cks = _gpu_session(n, cd, ticks, before=_lazy)
    d = cm.deferred_counts(g)
    assert d is not None and d[0] > ticks // 2, (d, g.kernel_info()["deferred_saves"])           # Saves were deferred: their checksum part came from the registers ...
    _compare(g, ids, cks, _reference(n, cd, ticks), "lazy live 3", cd)
    assert cm.deferred_counts(g)[1] > 0, g.kernel_info()["deferred_saves"]                       # ... and the ring frames just compared were replayed on demand


def test_knob_value_tags_on():
    n, cd, ticks = 300, 2, 40
    g, ids, cks = _gpu_session(n, cd, ticks, before=lambda w: w._lib.ggrs_dbg_set_value_tags(w._p, 1))
    assert g.kernel_info()["value_tags"].startswith("on"), g.kernel_info()["value_tags"]
    _compare(g, ids, cks, _reference(n, cd, ticks), "value tags", cd)


def test_knob_specialised_copies_forced_at_first_sight(monkeypatch):
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    n, cd, ticks = 300, 2, 40
    g, ids, cks = _gpu_session(n, cd, ticks, before=lambda w: w._lib.ggrs_dbg_set_spec_shapes(w._p, 3))
    assert g.kernel_info()["specialised_kernel"].startswith("ready"), g.kernel_info()["specialised_kernel"]
    _compare(g, ids, cks, _reference(n, cd, ticks), "specialised copies", cd)


def test_depth_parallel_roles_taken():
    """A SyncTest group of two and more Saves at this size is split over roles (blockIdx.y): every role replays the resource chain from the source block."""
    n, cd, ticks = 300, 2, 40
    g, ids, cks = _gpu_session(n, cd, ticks)
    assert int(g.kernel_info()["depth_parallel_roles"].split()[0]) > ticks // 2, g.kernel_info()["depth_parallel_roles"]
    _compare(g, ids, cks, _reference(n, cd, ticks), "depth-parallel roles", cd)


def test_host_edit_between_lists_and_rollbacks_around_it():
    """resource_write between lists -- once while the live block is lazily left unwritten --: a rollback to a frame before the edit restores the older value, one to a
    frame after it keeps the edit.  The model receives the same edit."""
    n = 300
    o = OracleWorld(n + 128, DEPTH, FLAT); model = rc.ClockModel(); _setup(o, n, model)
    g = bg.World(n + 128, max_depth=DEPTH); _lazy(g); _setup(g, n)
    g.set_synctest_check_distance(-1)
    a = lambda f: bg.AdvanceFrame(((f * 5 + 2) & 15,), dt_bits=rc.DT_BITS)      # noqa: E731

    def both(reqs):
        want = rc.run_model(o, model, reqs)
        got = list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], g.handle_requests(reqs)))
        assert got == want, (reqs, got, want)
        assert rc.read_resources(g) == model.words(), reqs

    def edit(clock, big):
        g.resource_write(0, clock); g.resource_write(2, [big])
        model.cur[0], model.cur[1], model.cur[3] = clock[0], clock[1], big
        assert rc.read_resources(g) == model.words()
    for f in range(3): both([bg.SaveGameState(f), a(f)])
    edit([1000, 99], 5 << 33)                                                                    # at frame 3, before its Save
    for f in range(3, 5): both([bg.SaveGameState(f), a(f)])
    both([bg.LoadGameState(4), a(4), bg.SaveGameState(5), a(5)])                                 # a frame after the edit: kept (ticks counts on from 1000)
    assert model.cur[0] == 1003
    both([bg.LoadGameState(2), a(2), bg.SaveGameState(3), a(3), bg.SaveGameState(4), a(4)])      # a frame before it: the older value is back, the edit is gone
    assert model.cur[0] == 5
    # ... and once during a lazy-live streak: lists that open with a Load and end [.., Save, Advance] leave the live block unwritten (knob 3)
    d0 = cm.deferred_counts(g)[0]
    both([bg.LoadGameState(3), a(3), bg.SaveGameState(4), a(4), bg.SaveGameState(5), a(5)])
    assert cm.deferred_counts(g)[0] > d0, g.kernel_info()["deferred_saves"]                      # (the knob took: the list deferred a Save and left the live block)
    edit([77, 3], 9)                                                                             # the live block is materialised first, then written
    both([bg.SaveGameState(6), a(6)])
    assert model.cur[0] == 78
    both([bg.LoadGameState(5), a(5), bg.SaveGameState(6), a(6)])
    assert model.cur[0] == 7


def _fanout_rank(q, lib_path):
    try:
        import os
        os.environ["GGRS_RCCL_LIB"] = lib_path
        import branch_marks_common as bm
        from bevy_ggrs_amd.fanout import RcclFanout
        n, depth, B, T, F = 300, 8, 4, 3, 3
        g = bg.World(n + 128, max_depth=depth); o = OracleWorld(n + 128, depth, FLAT); model = rc.ClockModel()
        ids = _setup(g, n); ido = _setup(o, n, model)
        dt = lambda f: rc.bits_f32(o._lib.gor_dt_bits(60, f))                   # noqa: E731  (a branch step derives Time::delta_secs from the frame: so do these lists)

        def walk(reqs, want):
            for r in reqs:
                if isinstance(r, bg.SaveGameState): model.save(r.frame)
                elif isinstance(r, bg.LoadGameState): model.load(r.frame)
                else: model.step(int(r.inputs[0]), dt(o.frame + 1))
                cs = o.handle_requests([r])
                if isinstance(r, bg.SaveGameState): want.append(cs[0] ^ model.part())
        warm = []
        for f in range(F):
            reqs = [bg.SaveGameState(f), bg.AdvanceFrame(((f + 2) & 15,))]
            g.handle_requests(reqs); walk(reqs, warm)
        native = RcclFanout(g, 0, 1, RcclFanout.unique_id())
        fold = g.kernel_info()["checksum_fold"]
        pred = (np.arange(B)[:, None] * 3 + np.arange(T)[None, :] * 5 + 1) % 7
        prefix = [bg.SaveGameState(F)]
        rc_keep, msg = bm.library_step(native, g, prefix, pred, _ffi.BRANCH_SAVE_LAST | _ffi.BRANCH_RETAIN_NEWEST)
        rcode, got = bm.library_step(native, g, prefix, pred, _ffi.BRANCH_SAVE_LAST)
        res_after = rc.read_resources(g)
        reqs = list(prefix)
        for b in range(B): reqs += bm.branch_requests(F, pred[b], T, True, T)
        reqs.append(bg.LoadGameState(F))
        ns = native.step(reqs)                                                 # ggrs_hip_fanout_step: k_gen_finalize and its device copy into the send buffer
        table = native.collect()
        listed = [int(p[0]) | (int(p[1]) << 64) for p in table.reshape(-1, 2)]
        want = []
        walk(reqs, want)
        confirmed = model.words(model.snaps[F])
        same = True
        try: cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), "fan-out")
        except AssertionError: same = False
        res_end = rc.read_resources(g)
        native.close()
        q.put(("ok", rc_keep, msg, rcode, got, ns, listed, want, same, res_after, res_end, confirmed, fold))
    except Exception as e:                                    # noqa: BLE001
        import traceback
        q.put(("error", f"{type(e).__name__}: {e}", traceback.format_exc()))


def test_branch_steps_without_retention_and_the_fanout_list_form():
    """ggrs_hip_fanout_step_branches, 4 branches x 3 frames with different inputs off one confirmed frame (each member runs its own resource chain in its own
    registers), against ggrs_hip_fanout_step's list form on the same world (k_gen_finalize, the device copy) and the oracle's walk with the model;
    GGRS_BRANCH_RETAIN_NEWEST is refused; afterwards the live world's resources are the confirmed frame's."""
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
    _, rc_keep, msg, rcode, got, ns, listed, want, same, res_after, res_end, confirmed, fold = r
    assert rc_keep == bg.GGRS_E_INVALID and "GGRS_BRANCH_RETAIN_" in msg and "device resources" in msg, (rc_keep, msg)
    assert fold == "k_gen_finalize", fold
    assert rcode == 0 and len(got) == 1 and len(got[0]) == 1 + 4 * 3, (rcode, got)
    assert ns == 1 + 4 * 3 and got[0] == listed == want, (ns, got, listed, want)
    assert len({tuple(got[0][1 + 3 * b: 4 + 3 * b]) for b in range(4)}) == 4                    # the branches diverge
    assert same and res_after == confirmed and res_end == confirmed, (same, res_after, res_end, confirmed)


def test_the_feature_adds_no_launch():
    """Over 20 steady SyncTest ticks at 8262 slots the clock world launches exactly as often as the same world with `tick` removed and `drift` reading a constant."""
    counts = {}
    for which in ("clock", "plain"):
        g = bg.World(8262 + 128, max_depth=DEPTH); ids = _setup(g, 8262, plain=which == "plain")
        g.set_synctest_check_distance(7)
        lists = rc.synctest_lists(7, 32, DEPTH)
        for reqs in lists[:12]: g.handle_requests(reqs)
        g.profile_enable(True)
        for reqs in lists[12:]: g.handle_requests(reqs)
        counts[which] = {k: v[1] for k, v in g.profile_read().items()}
        g.profile_enable(False)
    assert counts["clock"] == counts["plain"] and counts["clock"]["tick"] >= 20, counts
