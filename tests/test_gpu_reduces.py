"""Entity systems that reduce into a device resource (ggrs_hip_add_custom_system_reduces: e.reduce_u32 / _i32 / _u64 -- ResMut inside a query loop).  Everything goes
through the C ABI and is bit-exact: the Checksum(u128) of every SaveGameState equals the CPU oracle's XOR the resource parts of the Python model kept beside it
(reduces_common.ReduceModel; the oracle has no resources), the final state and every frame the ring holds equal the oracle's, resource_read of every resource equals
the model's value at that frame, and the reduce inbox holds identities whenever a host call has returned.

Shapes -- the smallest at which the reduction can go wrong: 1 slot (a single lane), 64 and 65 (the wave edge), 257 (two workgroups), 64 x 256 + 1 (workgroup 64
publishes into the inbox line of workgroup 0: the stripe index wraps; the slots between the first hundred and the last hold entities no user-written system visits,
so the oracle stays cheap), 1 048 646 for the in-place test (4097 workgroups; built-in systems and a handful of census entities on the oracle side).  An oracle session
is computed once per shape and shared, unchanged, by the tests that compare against it."""
import functools

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
import reduces_common as rd
from bevy_ggrs_amd import _ffi
from oracle.binding import FLAT, OracleWorld

pytestmark = pytest.mark.gpu
DEPTH = 8
U32 = np.uint32
WRAP = 64 * 256 + 1


def _shape(n):
    """(census entities in front, Fuse-only entities, census entities behind them, fuse base)"""
    if n == WRAP: return 100, WRAP - 101, 1, 5
    return n, 0, 0, (15 if n == 1 else 5)


def _setup(w, n, model=None, **kw):
    ids = rd.build_census(w, **({"model": model} if isinstance(w, OracleWorld) else {}), **kw)
    front, filler, tail, fuse_base = _shape(n)
    rd.spawn_census(w, ids, front, filler=filler, tail=tail, fuse_base=fuse_base)
    w.set_depth(DEPTH)
    return ids


def _ring_states(w, ids, resources=False):
    """Every frame the ring holds, loaded newest first (a Load pops the newer snapshots): the state and -- a library world -- the resources the Load restored."""
    out = {}
    for f in reversed([f for f in range(w.frame + 1) if w.has_snapshot(f)]):
        w.load(f)
        out[f] = (cm.snapshot_state(w, ids), rd.read_resources(w) if resources else None)
    return out


@functools.lru_cache(maxsize=None)
def _reference(n, cd, ticks):
    """The oracle's session with the model beside it: ([(frame, checksum ^ resource parts)], final state, {frame: state} of the ring, the model, its final values)."""
    o = OracleWorld(n + 128, DEPTH, FLAT)
    model = rd.census_model()
    ids = _setup(o, n, model)
    got = []
    for reqs in rd.synctest_lists(cd, ticks, DEPTH): rd.run_model(o, model, reqs, cd=cd, got=got)
    final = cm.snapshot_state(o, ids)
    if n > 1: assert 0 < int(final["alive"].sum()) < n, "entities die mid-session, not all of them"
    assert model.sent > 0
    cur = model.words()
    return got, final, {f: s for f, (s, _) in _ring_states(o, ids).items()}, model, cur


def _gpu_session(n, cd, ticks, *, before=None):
    g = bg.World(n + 128, max_depth=DEPTH)
    if before: before(g)
    ids = _setup(g, n)
    g.set_synctest_check_distance(cd)
    lists = rd.synctest_lists(cd, ticks, DEPTH)
    cks = []
    for reqs in lists: cks += g.handle_requests(reqs)
    frames = [r.frame for reqs in lists for r in reqs if isinstance(r, bg.SaveGameState)]
    advances = sum(isinstance(r, bg.AdvanceFrame) for reqs in lists for r in reqs)
    return g, ids, list(zip(frames, cks)), advances


def _compare(g, ids, cks, ref, ctx, cd):
    want, final, ring_states, model, cur = ref
    assert len(cks) == len(want) > 0, (len(cks), len(want))
    for (fa, ca), (fb, cb) in zip(cks, want):
        assert fa == fb and ca == cb, f"{ctx}: frame {fa}: gpu {ca:#x} oracle ^ model {cb:#x}"
    cm.assert_states_equal(cm.snapshot_state(g, ids), final, ctx)
    assert rd.read_resources(g) == cur, (ctx, rd.read_resources(g), cur)
    assert rd.inbox_is_identities(g, rd.CENSUS_LAYOUT), ctx
    got = _ring_states(g, ids, resources=True)
    assert sorted(got) == sorted(ring_states) and len(got) >= min(cd, 2), (sorted(got), sorted(ring_states))
    for f, (state, res) in got.items():
        cm.assert_states_equal(state, ring_states[f], f"{ctx}: ring frame {f}")
        assert res == model.words(model.snaps[f]), (ctx, f, res, model.words(model.snaps[f]))


def _applies(g):
    return int(g.kernel_info()["reduce_inbox"].split("(")[1].split()[0])


def _is_reduce_world(g, stripes=64, words=4):
    """The host policy of such a world: one AdvanceWorld per launch, no lazy live block, no deferred Saves."""
    info = g.kernel_info()
    assert info["request_group_kernel"].startswith("ggrs_jit_tick"), info
    assert info["group_caps"].endswith("/ 1 steps") and info["deferred_saves"].startswith("off"), info
    assert info["reduce_inbox"].startswith(f"{stripes} stripes of 64 bytes laid out like a resource cell, {words} reduced words"), info["reduce_inbox"]
    assert info["device_resources"].startswith("3 resources, 20 bytes"), info


@pytest.mark.parametrize("n", [1, 64, 65, 257, WRAP])
@pytest.mark.parametrize("cd", [2, 7])
def test_census_synctest_against_the_oracle_and_the_model(n, cd):
    ticks = 24
    ref = _reference(n, cd, ticks)
    g, ids, cks, advances = _gpu_session(n, cd, ticks)
    _is_reduce_world(g)
    assert _applies(g) == advances, (g.kernel_info()["reduce_inbox"], advances)      # one apply per AdvanceFrame request executed, none lazily
    _compare(g, ids, cks, ref, f"census {n} cd {cd}", cd)


def test_p2p_shaped_rollbacks_whose_inputs_change_between_prediction_and_confirmation():
    """Rollbacks of 0 to 7 frames; a re-simulated frame sees another input than its first simulation, so `wound` and with it every reduction differs: a wrong restore
    of the never-reset Total, or an inbox that kept something of the predicted frame, shows."""
    n = 300
    lists = rd.p2p_lists(36)
    assert {len([r for r in reqs if isinstance(r, bg.AdvanceFrame)]) - 1 for _, reqs in lists} == set(range(8))
    o = OracleWorld(n + 128, DEPTH, FLAT); model = rd.census_model(); ido = _setup(o, n, model)
    g = bg.World(n + 128, max_depth=DEPTH); ids = _setup(g, n)
    g.set_synctest_check_distance(-1)
    want, got, advances = [], [], 0
    for confirmed, reqs in lists:
        rd.run_model(o, model, reqs, confirmed=confirmed, got=want)
        if confirmed is not None: g.set_confirmed(confirmed)
        cs = g.handle_requests(reqs)
        advances += sum(isinstance(r, bg.AdvanceFrame) for r in reqs)
        got += list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], cs))
    assert got == want and len(got) > 100
    cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), "p2p-shaped lists")
    assert rd.read_resources(g) == model.words() and rd.inbox_is_identities(g, rd.CENSUS_LAYOUT) and _applies(g) == advances
    rg, ro = _ring_states(g, ids, resources=True), _ring_states(o, ido)
    assert sorted(rg) == sorted(ro) and len(rg) >= 7
    for f in rg:
        cm.assert_states_equal(rg[f][0], ro[f][0], f"p2p ring frame {f}")
        assert rg[f][1] == model.words(model.snaps[f]), f


@pytest.mark.parametrize("wb", [4, 8])
def test_all_eight_ops_on_words_of_one_width(wb):
    """130 slots; word k of the resource under op k, every entity sends its LCG value into all eight every frame: MIN_I / MAX_I over values of both signs, an ADD
    that wraps; `mix` puts the identities back on odd inputs, so AND / OR / MIN / MAX are tested frame by frame and across frames.  The accessors of the other
    width, called beside them, do nothing."""
    n, cd = 130, 2
    layout = rd.ops_layout(wb)
    o = OracleWorld(n + 64, DEPTH, FLAT); model = rd.ReduceModel(layout, rd.ops_mix(wb)); ido = rd.build_ops(o, wb, model=model)
    g = bg.World(n + 64, max_depth=DEPTH); ids = rd.build_ops(g, wb)
    init = (np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(U32)
    for w, wi in ((o, ido), (g, ids)): w.spawn(n, {wi[0]: [init]}); w.set_depth(DEPTH)
    g.set_synctest_check_distance(cd)
    want, got, wrapped, signs = [], [], False, set()
    for reqs in rd.synctest_lists(cd, 16, DEPTH):
        for r in reqs:
            if isinstance(r, bg.AdvanceFrame):
                vals = [rd._feed_value(int(v), wb) for v in (o.download_word(ido[0], 0, 0, n).astype(np.uint64) * 1664525 + 1013904223 + int(r.inputs[0])) % (1 << 32)]
                wrapped |= sum(vals) >= 1 << (8 * wb); signs |= {v >> (8 * wb - 1) for v in vals}
            rd.run_model(o, model, [r], cd=cd, got=want)
        cs = g.handle_requests(reqs)
        got += list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], cs))
        assert rd.read_resources(g, 1) == model.words(), (rd.read_resources(g, 1), model.words())
    assert got == want and len(got) > 20 and wrapped and signs == {0, 1}
    assert rd.inbox_is_identities(g, layout)
    assert g.kernel_info()["reduce_inbox"].startswith("64 stripes of 64 bytes laid out like a resource cell, 8 reduced words")
    cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), f"ops {wb}")


def test_a_frame_in_which_no_lane_reduces_leaves_the_word_as_the_resource_system_left_it():
    """Every entity's fuse runs out at frame 2: from then on the systems run for nobody.  alive = 0, flags = input << 16 and hp = 0xFFFFFFFF are what `reset` left, Total
    keeps what it had, and the inbox is all identities."""
    n = 130
    g = bg.World(n + 64, max_depth=DEPTH); ids = rd.build_census(g)
    rd.spawn_census(g, ids, n, fuse_base=2, fuse_mod=1); g.set_depth(DEPTH)
    g.set_synctest_check_distance(-1)
    total = None
    for f in range(5):
        g.handle_requests([bg.SaveGameState(f), bg.AdvanceFrame(((f + 3) & 15,), dt_bits=rd.DT_BITS)])
        census, low, tot = rd.read_resources(g)
        assert rd.inbox_is_identities(g, rd.CENSUS_LAYOUT), f
        if f < 2:
            assert census[0] == n and census[1] & 0xFFFF0000 == ((f + 3) & 15) << 16 and low[0] < 0xFFFFFFFF, (f, census, low)
            total = tot
        else:
            assert census == [0, ((f + 3) & 15) << 16] and low == [0xFFFFFFFF] and tot == total, (f, census, low, tot, total)
    assert total[0] > rd.TOTAL_INIT and int(cm.snapshot_state(g, ids)["alive"].sum()) == 0


def test_a_reducer_that_despawns_its_own_entity_in_the_same_call_still_counts():
    n = 130
    layout = [("Tally", 4, [(0, bg.EFFECT_ADD), (0, bg.EFFECT_MAX_U)])]
    src = ("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) { e.u32(0) -= 1u; e.reduce_u32(0, 1u); "
           "if (e.u32(0) < 40u + (ggrs_u32)f.input[0]) { e.reduce_u32(1, (ggrs_u32)e.slot); e.despawn(); } }")
    o = OracleWorld(n + 64, DEPTH, FLAT); model = rd.ReduceModel(layout)
    g = bg.World(n + 64, max_depth=DEPTH)
    ido = (o.register_component("Hp", 4, 1),); ids = (g.register_component("Hp", 4, 1),)
    o.checksum_component(ido[0], [0]); g.checksum_component(ids[0], [0])

    def leave(words, slot, f):
        hp = (words[0] - 1) & rd.M32
        model.reduce(0, 0, 1)
        if hp < 40 + f.input(0)[0]: model.reduce(0, 1, slot); return [hp], 1
        return [hp], 0
    o.add_custom_system(leave, [(ido[0], 0)])
    (T,) = rd.register_model_resources(g, model)
    g.add_custom_system(src, [(ids[0], 0)], name="leave", reduces=[(T, 0, bg.EFFECT_ADD), (T, 1, bg.EFFECT_MAX_U)])
    hp0 = (45 + (np.arange(n) * 7) % 23).astype(U32)
    for w, wi in ((o, ido), (g, ids)): w.spawn(n, {wi[0]: [hp0]}); w.set_depth(DEPTH)
    g.set_synctest_check_distance(2)
    want, got, alive = [], [], []
    for reqs in rd.synctest_lists(2, 14, DEPTH):
        rd.run_model(o, model, reqs, cd=2, got=want)
        got += list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], g.handle_requests(reqs)))
        assert rd.read_resources(g, 1) == model.words()
        alive.append(int(cm.snapshot_state(o, ido)["alive"].sum()))
    assert got == want and alive[0] > alive[-1] and model.cur[0][1] > 0        # entities left mid-session, and the slot of one that left is in the MAX_U word
    cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), "leave")
    assert rd.inbox_is_identities(g, layout)


def _big_lists():
    """Plain ticks (live -> live, no Load) and lists in which a Save lands on the slot the group loaded: Load(F) pops F's slot, Save(F) takes it back."""
    a = lambda f: bg.AdvanceFrame(((f * 3 + 1) & 15,), dt_bits=rd.DT_BITS)      # noqa: E731
    return [[bg.SaveGameState(0), a(0)], [bg.SaveGameState(1), a(1)], [bg.SaveGameState(2), a(2)],
            [bg.LoadGameState(2), bg.SaveGameState(2), a(2), bg.SaveGameState(3), a(3)],
            [bg.SaveGameState(4), a(4)], [bg.LoadGameState(4), bg.SaveGameState(4), a(4)], [bg.SaveGameState(5), a(5)]]


def test_in_place_launches_at_4097_workgroups():
    """live -> live and a Save into the slot the group loaded, with a grid of 4097 workgroups and `count` registered: 70 census entities in workgroup 0 and 6 in the
    last workgroup (slots from 1 048 640), which publishes into inbox line 4096 mod 64 = 0 like workgroup 0; k_apply_reduces writes the cell the launch made current."""
    n = 1_048_646
    o = OracleWorld(n + 64, 4, FLAT); model = rd.census_model(); ido = rd.build_big(o, model=model)
    g = bg.World(n + 64, max_depth=4); ids = rd.build_big(g)
    init = (np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(U32)
    for w, (A, Hp) in ((o, ido), (g, ids)):
        w.spawn(70, {A: [init[:70]], Hp: [(1000 + np.arange(70) * 13).astype(U32)]})
        w.spawn(n - 76, {A: [init[70:n - 6]]})
        w.spawn(6, {A: [init[n - 6:]], Hp: [(900 + np.arange(6) * 5).astype(U32)]})
        w.set_depth(4)
    g.set_synctest_check_distance(-1)
    for k, reqs in enumerate(_big_lists()):
        want = rd.run_model(o, model, reqs)
        cs = g.handle_requests(reqs)
        got = list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], cs))
        assert got == want, (k, got, want)
        assert rd.read_resources(g) == model.words(), (k, rd.read_resources(g), model.words())
    assert model.cur[0][0] == 76 and model.cur[1][0] == 900
    assert (g.download_word(ids[0], 0, n - 5, 5) == o.download_word(ido[0], 0, n - 5, 5)).all() and g.frame == 6
    assert rd.inbox_is_identities(g, rd.CENSUS_LAYOUT)
    for f in (5, 4):
        g.load(f)
        assert rd.read_resources(g) == model.words(model.snaps[f]), f


def test_host_resource_write_between_lists_with_rollbacks_around_it():
    """resource_write between lists: a rollback to a frame before the edit restores the older Total, one to a frame after it keeps the edit and the reductions
    go on top of it.  The model receives the same edit."""
    n = 257
    o = OracleWorld(n + 128, DEPTH, FLAT); model = rd.census_model(); _setup(o, n, model)
    g = bg.World(n + 128, max_depth=DEPTH); _setup(g, n)
    g.set_synctest_check_distance(-1)
    a = lambda f: bg.AdvanceFrame(((f * 5 + 2) & 15,), dt_bits=rd.DT_BITS)      # noqa: E731

    def both(reqs):
        want = rd.run_model(o, model, reqs)
        got = list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], g.handle_requests(reqs)))
        assert got == want, (reqs, got, want)
        assert rd.read_resources(g) == model.words(), reqs

    def edit(total, low):
        g.resource_write(2, [total]); g.resource_write(1, [low])
        model.cur[2][0], model.cur[1][0] = total, low
        assert rd.read_resources(g) == model.words()
    for f in range(3): both([bg.SaveGameState(f), a(f)])
    edit(5 << 56, 3)                                                                             # at frame 3, before its Save
    for f in range(3, 5): both([bg.SaveGameState(f), a(f)])
    assert model.cur[2][0] > 5 << 56
    both([bg.LoadGameState(4), a(4), bg.SaveGameState(5), a(5)])                                 # a frame after the edit: kept
    assert 5 << 56 < model.cur[2][0] < 6 << 56
    both([bg.LoadGameState(2), a(2), bg.SaveGameState(3), a(3), bg.SaveGameState(4), a(4)])      # a frame before it: the older value is back, the edit is gone
    assert rd.TOTAL_INIT < model.cur[2][0] < 5 << 56
    assert rd.inbox_is_identities(g, rd.CENSUS_LAYOUT)


def test_knob_specialised_copies_forced_at_first_sight(monkeypatch):
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    n, cd, ticks = 257, 2, 24
    g, ids, cks, _ = _gpu_session(n, cd, ticks, before=lambda w: w._lib.ggrs_dbg_set_spec_shapes(w._p, 4))
    assert g.kernel_info()["specialised_kernel"].startswith("ready"), g.kernel_info()["specialised_kernel"]
    _compare(g, ids, cks, _reference(n, cd, ticks), "specialised copies", cd)


def test_knob_value_tags_on():
    """Value tags stay available to such a world (k_apply_reduces touches no column): forced on here."""
    n, cd, ticks = 257, 2, 24
    g, ids, cks, _ = _gpu_session(n, cd, ticks, before=lambda w: w._lib.ggrs_dbg_set_value_tags(w._p, 1))
    assert g.kernel_info()["value_tags"].startswith("on"), g.kernel_info()["value_tags"]
    _compare(g, ids, cks, _reference(n, cd, ticks), "value tags", cd)


def test_one_stripe():
    """One inbox line instead of 64: both workgroups publish into it, lanes 1..63 of k_apply_reduces fold identities."""
    n, cd, ticks = 257, 2, 24
    g, ids, cks, _ = _gpu_session(n, cd, ticks, before=lambda w: w._lib.ggrs_dbg_set_reduce_stripes(w._p, 1))
    _is_reduce_world(g, stripes=1)
    _compare(g, ids, cks, _reference(n, cd, ticks), "one stripe", cd)


def _fanout_rank(q, lib_path):
    try:
        import os
        os.environ["GGRS_RCCL_LIB"] = lib_path
        import branch_marks_common as bm
        from bevy_ggrs_amd.fanout import RcclFanout
        n, depth, B, T, F = 257, 8, 4, 3, 3
        g = bg.World(n + 128, max_depth=depth); o = OracleWorld(n + 128, depth, FLAT); model = rd.census_model()
        ids = _setup(g, n); ido = _setup(o, n, model)
        warm = []
        for f in range(F):
            reqs = [bg.SaveGameState(f), bg.AdvanceFrame(((f + 2) & 15,))]
            g.handle_requests(reqs); rd.run_model(o, model, reqs, got=warm)
        native = RcclFanout(g, 0, 1, RcclFanout.unique_id())
        pred = (np.arange(B)[:, None] * 3 + np.arange(T)[None, :] * 5 + 1) % 7
        prefix = [bg.SaveGameState(F)]
        rcode, msg = bm.library_step(native, g, prefix, pred, _ffi.BRANCH_SAVE_LAST)
        reqs = list(prefix)
        for b in range(B): reqs += bm.branch_requests(F, pred[b], T, True, T)
        reqs.append(bg.LoadGameState(F))
        ns = native.step(reqs)                                                 # ggrs_hip_fanout_step: the list form
        table = native.collect()
        listed = [int(p[0]) | (int(p[1]) << 64) for p in table.reshape(-1, 2)]
        want = [c for _, c in rd.run_model(o, model, reqs)]
        confirmed = model.words(model.snaps[F])
        same = True
        try: cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), "fan-out")
        except AssertionError: same = False
        res_end = rd.read_resources(g)
        clean = rd.inbox_is_identities(g, rd.CENSUS_LAYOUT)
        native.close()
        q.put(("ok", rcode, msg, ns, listed, want, same, res_end, confirmed, clean))
    except Exception as e:                                    # noqa: BLE001
        import traceback
        q.put(("error", f"{type(e).__name__}: {e}", traceback.format_exc()))


def test_fanout_step_works_and_branch_steps_are_refused():
    """ggrs_hip_fanout_step_branches is refused with a message; ggrs_hip_fanout_step's list form -- 4 branches x 3 frames with different inputs off one confirmed frame,
    each frame its own launch and apply -- equals the oracle's walk with the model; afterwards the live world's resources are the confirmed frame's."""
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
    _, rcode, msg, ns, listed, want, same, res_end, confirmed, clean = r
    assert rcode == bg.GGRS_E_INVALID and "ggrs_hip_fanout_step_branches" in msg and "reduce bindings" in msg and "ggrs_hip_fanout_step" in msg, (rcode, msg)
    assert ns == 1 + 4 * 3 and listed == want, (ns, listed, want)
    assert len({tuple(listed[1 + 3 * b: 4 + 3 * b]) for b in range(4)}) == 4                     # the branches diverge
    assert same and res_end == confirmed and clean, (same, res_end, confirmed, clean)
