"""Deterministic float sums into a device resource (ggrs_hip_add_custom_system_sums: e.sum_f32 / e.sum_f64).  Everything goes through the C ABI and is compared as
BITS: the Checksum(u128) of every SaveGameState equals the CPU oracle's XOR the resource parts of the Python model kept beside it (sums_common.SumModel: per-slot
pending values at -0.0, the frame total by the balanced binary tree over slot indices, one add into the word; the oracle has no resources), the final state and every
frame the ring holds equal the oracle's, and resource_read of every resource equals the model's bits at that frame.  The flock's starting values make the ORDER of a
float sum show (test_sums_text.py asserts it for these sizes): a sum in slot order, in arrival order, or per wave then sequentially gives other bits.

Shapes -- the smallest at which the sum can go wrong: 1 slot (a single lane), 63 / 64 / 65 (the wave edge), 256 / 257 (the workgroup edge), 1025 (five workgroups: a
count that is no power of two), 1 048 646 for the in-place test (4097 workgroups, 16 386 units: k_apply_sums runs two 16-to-1 passes through both of its buffers and
then the levels in LDS; built-in systems and a handful of flock entities on the oracle side).  An oracle session is computed once per shape and shared, unchanged."""
import functools

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
import reduces_common as rd
import sums_common as sc
from bevy_ggrs_amd import _ffi
from oracle.binding import FLAT, OracleWorld

pytestmark = pytest.mark.gpu
DEPTH = 8
U32 = np.uint32
TICKS = 14


def _setup(w, n, model=None, **kw):
    ids = sc.build_flock(w, **({"model": model} if isinstance(w, OracleWorld) else {}), **kw)
    sc.spawn_flock(w, ids, n, fuse_base=(9 if n == 1 else 5), fuse_mod=(1 if n == 1 else 17))
    w.set_depth(DEPTH)
    return ids


def _ring_states(w, ids, resources=False):
    """Every frame the ring holds, loaded newest first (a Load pops the newer snapshots): the state and -- a library world -- the resources the Load restored."""
    out = {}
    for f in reversed([f for f in range(w.frame + 1) if w.has_snapshot(f)]):
        w.load(f)
        out[f] = (cm.snapshot_state(w, ids), sc.read_resources(w) if resources else None)
    return out


@functools.lru_cache(maxsize=None)
def _reference(n, cd, ticks):
    """The oracle's session with the model beside it: ([(frame, checksum ^ resource parts)], final state, {frame: state} of the ring, the model, its final words)."""
    o = OracleWorld(n + 128, DEPTH, FLAT)
    model = sc.flock_model(n + 128)
    ids = _setup(o, n, model)
    got, per_list = [], []
    for reqs in rd.synctest_lists(cd, ticks, DEPTH):
        rd.run_model(o, model, reqs, cd=cd, got=got)
        per_list.append(model.words())
    final = cm.snapshot_state(o, ids)
    alive = int(final["alive"].sum())
    assert (0 < alive < n) if n > 1 else alive == 0, "entities die mid-session"
    assert model.sent > 0
    return got, final, {f: s for f, (s, _) in _ring_states(o, ids).items()}, model, per_list


def _gpu_session(n, cd, ticks, *, before=None):
    g = bg.World(n + 128, max_depth=DEPTH)
    if before: before(g)
    ids = _setup(g, n)
    g.set_synctest_check_distance(cd)
    lists = rd.synctest_lists(cd, ticks, DEPTH)
    cks, per_list = [], []
    for reqs in lists:
        cks += g.handle_requests(reqs)
        per_list.append(sc.read_resources(g))
    frames = [r.frame for reqs in lists for r in reqs if isinstance(r, bg.SaveGameState)]
    advances = sum(isinstance(r, bg.AdvanceFrame) for reqs in lists for r in reqs)
    return g, ids, list(zip(frames, cks)), advances, per_list


def _compare(g, ids, cks, per_list, ref, ctx, cd):
    want, final, ring_states, model, want_lists = ref
    assert per_list == want_lists, (ctx, [k for k, (a, b) in enumerate(zip(per_list, want_lists)) if a != b][:3])       # every resource word's bits after every list
    assert len(cks) == len(want) > 0, (len(cks), len(want))
    for (fa, ca), (fb, cb) in zip(cks, want):
        assert fa == fb and ca == cb, f"{ctx}: frame {fa}: gpu {ca:#x} oracle ^ model {cb:#x}"
    cm.assert_states_equal(cm.snapshot_state(g, ids), final, ctx)
    got = _ring_states(g, ids, resources=True)
    assert sorted(got) == sorted(ring_states) and len(got) >= min(cd, 2), (sorted(got), sorted(ring_states))
    for f, (state, res) in got.items():
        cm.assert_states_equal(state, ring_states[f], f"{ctx}: ring frame {f}")
        assert res == model.words(model.snaps[f]), (ctx, f, res, model.words(model.snaps[f]))


def _applies(g):
    return int(g.kernel_info()["sum_partials"].split("(")[1].split()[0])


def _is_sum_world(g, units):
    """The host policy of such a world: one AdvanceWorld per launch, no lazy live block, no deferred Saves."""
    info = g.kernel_info()
    assert info["request_group_kernel"].startswith("ggrs_jit_tick"), info
    assert info["group_caps"].endswith("/ 1 steps") and info["deferred_saves"].startswith("off"), info
    assert info["sum_partials"].startswith(f"{units} units of 64 slots, 3 summed words"), info["sum_partials"]
    assert info["device_resources"].startswith("3 resources, 20 bytes"), info


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1025])
@pytest.mark.parametrize("cd", [2, 7])
def test_flock_synctest_against_the_oracle_and_the_model(n, cd):
    ref = _reference(n, cd, TICKS)
    g, ids, cks, advances, per_list = _gpu_session(n, cd, TICKS)
    _is_sum_world(g, 128)
    assert _applies(g) == advances, (g.kernel_info()["sum_partials"], advances)        # one fold per AdvanceFrame request executed, none lazily
    _compare(g, ids, cks, per_list, ref, f"flock {n} cd {cd}", cd)


def test_p2p_shaped_rollbacks_whose_inputs_change_between_prediction_and_confirmation():
    """Rollbacks of 0 to 7 frames; a re-simulated frame sees another input than its first simulation, so `steer` moves by another step and every sum differs: a wrong
    restore of the never-reset Energy, or a partial of the predicted frame that survived, shows.  A frame re-simulated with the SAME input reproduces its bits."""
    n = 300
    lists = rd.p2p_lists(36)
    assert {len([r for r in reqs if isinstance(r, bg.AdvanceFrame)]) - 1 for _, reqs in lists} == set(range(8))
    o = OracleWorld(n + 128, DEPTH, FLAT); model = sc.flock_model(n + 128); ido = _setup(o, n, model)
    g = bg.World(n + 128, max_depth=DEPTH); ids = _setup(g, n)
    g.set_synctest_check_distance(-1)
    want, got, advances = [], [], 0
    for confirmed, reqs in lists:
        rd.run_model(o, model, reqs, confirmed=confirmed, got=want)
        if confirmed is not None: g.set_confirmed(confirmed)
        cs = g.handle_requests(reqs)
        advances += sum(isinstance(r, bg.AdvanceFrame) for r in reqs)
        got += list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], cs))
        assert sc.read_resources(g) == model.words()
    assert got == want and len(got) > 100
    cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), "p2p-shaped lists")
    assert _applies(g) == advances
    rg, ro = _ring_states(g, ids, resources=True), _ring_states(o, ido)
    assert sorted(rg) == sorted(ro) and len(rg) >= 7
    for f in rg:
        cm.assert_states_equal(rg[f][0], ro[f][0], f"p2p ring frame {f}")
        assert rg[f][1] == model.words(model.snaps[f]), f


DRIP_SRC = ("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) { if (f.input[0] & 1) { e.sum_f32(0, e.f32(0)); e.sum_f32(1, e.f32(0)); "
            "e.sum_f64(2, (double)e.f32(0)); e.sum_f64(3, (double)e.f32(0)); e.sum_f64(0, 1.0); e.sum_f32(2, 1.f); } }")


def test_a_frame_in_which_no_lane_sums_leaves_the_words_bits_alone():
    """Words holding +0.0 and -0.0, float and double, no resource system.  Frames with an even input: the system runs and sums nothing; after frame 3 every entity is
    dead and the system runs for nobody.  In both cases T = -0.0 and w + T is w bit for bit.  The frame with an odd input, in between, changes all four words; an
    accessor of the other width does nothing."""
    n = 130
    layout = [("Z", 4, [(0, sc.SUM), (sc.NEG_ZERO_32, sc.SUM)]), ("D", 8, [(sc.NEG_ZERO_64, sc.SUM), (0, sc.SUM)])]
    o = OracleWorld(n + 64, DEPTH, FLAT); model = sc.SumModel(layout, n + 64)
    g = bg.World(n + 64, max_depth=DEPTH)
    ido = (o.register_component("V", 4, 1), o.register_component("Fuse", 4, 1)); ids = (g.register_component("V", 4, 1), g.register_component("Fuse", 4, 1))
    for w, wi in ((o, ido), (g, ids)): w.checksum_component(wi[0], [0]); w.checksum_component(wi[1], [0])

    def drip(words, slot, f):
        if f.input(0)[0] & 1:
            v = sc.bits_f32(words[0])
            model.sum(0, 0, slot, v); model.sum(0, 1, slot, v); model.sum(1, 0, slot, v); model.sum(1, 1, slot, v)
        return list(words), 0
    o.add_custom_system(drip, [(ido[0], 0)])
    Z, D = sc.register_model_resources(g, model)
    g.add_custom_system(DRIP_SRC, [(ids[0], 0)], name="drip", sums=[(Z, 0), (Z, 1), (D, 0), (D, 1)])
    for w, wi in ((o, ido), (g, ids)):
        w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(wi[1],), word=(0,), iparam=(1, bg.DESPAWN_IMMEDIATE))
        w.spawn(n, {wi[0]: [sc.order_values(n).view(U32)], wi[1]: [np.full(n, 4, dtype=U32)]}); w.set_depth(DEPTH)
    g.set_synctest_check_distance(-1)
    init = ([0, sc.NEG_ZERO_32], [sc.NEG_ZERO_64, 0])
    inputs = [2, 4, 3, 0, 1, 5, 6]
    want, got, seen = [], [], []
    for f, inp in enumerate(inputs):
        reqs = rd.stamp([[bg.SaveGameState(f), bg.AdvanceFrame((inp,))]])[0]
        rd.run_model(o, model, reqs, got=want)
        got += list(zip([f], g.handle_requests(reqs)))
        seen.append(sc.read_resources(g, 2))
        assert seen[-1] == model.words(), (f, seen[-1], model.words())
    assert got == want
    assert seen[0] == init and seen[1] == init, seen[:2]                                    # the system ran for 130 entities and summed nothing
    assert seen[2] != init and all(a != b for r0, r1 in zip(seen[2], init) for a, b in zip(r0, r1))
    assert int(cm.snapshot_state(g, ids)["alive"].sum()) == 0
    assert seen[3] == seen[2] and seen[4] == seen[2] and seen[6] == seen[2]               # ... and later for nobody, odd inputs included


def test_a_summer_that_despawns_its_own_entity_in_the_same_call_still_contributes():
    n = 130
    layout = [("Tally", 4, [(0, sc.SUM), (0, sc.SUM)])]
    src = ("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) { e.f32(0) = e.f32(0) - 1.f; e.sum_f32(0, e.f32(0)); "
           "if (e.f32(0) < 40.f + (float)f.input[0]) { e.sum_f32(1, e.f32(0) * 0.37f); e.despawn(); } }")
    o = OracleWorld(n + 64, DEPTH, FLAT); model = sc.SumModel(layout, n + 64)
    g = bg.World(n + 64, max_depth=DEPTH)
    ido = (o.register_component("Hp", 4, 1),); ids = (g.register_component("Hp", 4, 1),)
    o.checksum_component(ido[0], [0]); g.checksum_component(ids[0], [0])

    def leave(words, slot, f):
        hp = sc.bits_f32(words[0]) - sc.F32(1)
        model.sum(0, 0, slot, hp)
        if hp < sc.F32(40) + sc.F32(f.input(0)[0]): model.sum(0, 1, slot, hp * sc.F32(0.37)); return [sc.f32_bits(hp)], 1
        return [sc.f32_bits(hp)], 0
    o.add_custom_system(leave, [(ido[0], 0)])
    (T,) = sc.register_model_resources(g, model)
    g.add_custom_system(src, [(ids[0], 0)], name="leave", sums=[(T, 0), (T, 1)])
    hp0 = (sc.F32(45.3) + ((np.arange(n) * 7) % 23).astype(sc.F32) * sc.F32(1.37)).astype(sc.F32)
    for w, wi in ((o, ido), (g, ids)): w.spawn(n, {wi[0]: [hp0.view(U32)]}); w.set_depth(DEPTH)
    g.set_synctest_check_distance(2)
    want, got, alive, left = [], [], [], []
    for reqs in rd.synctest_lists(2, 14, DEPTH):
        rd.run_model(o, model, reqs, cd=2, got=want)
        got += list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], g.handle_requests(reqs)))
        assert sc.read_resources(g, 1) == model.words()
        alive.append(int(cm.snapshot_state(o, ido)["alive"].sum())); left.append(model.cur[0][1])
    assert got == want and alive[0] > alive[-1] and len(set(left)) > 3                     # entities left mid-session, and what they summed while leaving arrived
    cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), "leave")


# ---- big: the in-place world ----------------------------------------------------------------------------------------------------------------------------------
def _build_big(w, model=None):
    """Every entity has Acc (GGRS_SYS_ADD_U32: built-in on both sides); the few flock entities also have Pos, which `tally` sums."""
    A = w.register_component("Acc", 4, 1); Pos = w.register_component("Pos", 4, 2)
    w.checksum_component(A, [0]); w.checksum_component(Pos, [0, 1])
    w.add_system(bg.SYS_ADD_U32, comp=(A,), word=(0,), iparam=(3,))
    if isinstance(w, OracleWorld):
        def tally(words, slot, f):
            x, y = sc.bits_f32(words[0]), sc.bits_f32(words[1])
            model.sum(0, 0, slot, x); model.sum(0, 1, slot, y); model.sum(1, 0, slot, sc.F64(x) * sc.F64(x)); model.reduce(2, 0, 1)
            return list(words), 0
        w.add_custom_system(tally, [(Pos, 0), (Pos, 1)])
    else:
        Ce, En, Cn = sc.register_model_resources(w, sc.flock_model(1))
        w.add_resource_system(sc.RESET_SRC, [(Ce, 0), (Ce, 1), (Cn, 0)], name="reset")
        w.add_custom_system(sc.TALLY_SRC, [(Pos, 0), (Pos, 1)], name="tally", reduces=[(Cn, 0, bg.EFFECT_ADD)], sums=[(Ce, 0), (Ce, 1), (En, 0)])
    return A, Pos


def _big_lists():
    """Plain ticks (live -> live, no Load) and lists in which a Save lands on the slot the group loaded: Load(F) pops F's slot, Save(F) takes it back."""
    a = lambda f: bg.AdvanceFrame(((f * 3 + 1) & 15,), dt_bits=rd.DT_BITS)      # noqa: E731
    return [[bg.SaveGameState(0), a(0)], [bg.SaveGameState(1), a(1)], [bg.SaveGameState(2), a(2)],
            [bg.LoadGameState(2), bg.SaveGameState(2), a(2), bg.SaveGameState(3), a(3)],
            [bg.SaveGameState(4), a(4)], [bg.LoadGameState(4), bg.SaveGameState(4), a(4)], [bg.SaveGameState(5), a(5)]]


def test_in_place_launches_at_4097_workgroups():
    """live -> live and a Save into the slot the group loaded, with a grid of 4097 workgroups and `tally` registered: 70 flock entities in workgroup 0 (units 0 and 1)
    and 6 in the last workgroup (unit 16 385, slots from 1 048 640); a million filler entities between them that no user-written system visits.  The frame total
    pairs the head's sub-tree with the tail's only at the root of a 2^15-unit tree: the cross-workgroup levels of k_apply_sums run for real."""
    n = 1_048_646
    o = OracleWorld(n + 64, 4, FLAT); model = sc.flock_model(n + 64); ido = _build_big(o, model)
    g = bg.World(n + 64, max_depth=4); ids = _build_big(g)
    init = (np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(U32)
    xh, yh = sc.flock_xy(0, 70); xt, yt = sc.flock_xy(70, 6)
    for w, (A, Pos) in ((o, ido), (g, ids)):
        w.spawn(70, {A: [init[:70]], Pos: [xh.view(U32), yh.view(U32)]})
        w.spawn(n - 76, {A: [init[70:n - 6]]})
        w.spawn(6, {A: [init[n - 6:]], Pos: [xt.view(U32), yt.view(U32)]})
        w.set_depth(4)
    g.set_synctest_check_distance(-1)
    for k, reqs in enumerate(_big_lists()):
        want = rd.run_model(o, model, reqs)
        cs = g.handle_requests(reqs)
        got = list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], cs))
        assert got == want, (k, got, want)
        assert sc.read_resources(g) == model.words(), (k, sc.read_resources(g), model.words())
    assert model.cur[2][0] == 76
    # head + tail in the tree's order is not the slot-order sum of the 76 values: the total really went through the levels
    x = np.concatenate([xh, xt])
    assert model.cur[0][0] == sc.f32_bits(sc.tree_sum(xh) + sc.tree_sum(xt)) and model.cur[0][0] != sc.f32_bits(sc.seq_sum(x))
    info = g.kernel_info()["sum_partials"]
    assert info.startswith("16512 units of 64 slots, 3 summed words"), info
    parts = sc.sum_partials(g, 0, 16386)
    assert int(parts[16385]) & 0xFFFFFFFF == sc.f32_bits(sc.tree_sum(xt)) and int(parts[7]) & 0xFFFFFFFF == sc.NEG_ZERO_32 and int(parts[0]) & 0xFFFFFFFF == sc.f32_bits(sc.tree_sum(xh[:64]))
    assert (g.download_word(ids[0], 0, n - 5, 5) == o.download_word(ido[0], 0, n - 5, 5)).all() and g.frame == 6
    for f in (5, 4):
        g.load(f)
        assert sc.read_resources(g) == model.words(model.snaps[f]), f


def test_a_smaller_launch_never_reads_the_partials_of_an_earlier_larger_one():
    """65 entities, one frame; then 300 more are spawned and a frame covers 6 units, whose waves store real values into entries 2 .. 5 of the partial arrays; a Load
    of frame 0 brings len back to 65 and, once the larger blocks are rewritten, the launches cover 2 units again.  Every total is that of the entities the frame has:
    k_apply_sums folds the units ITS launch covered and nothing beyond (the entries there are zero bytes, +0.0, from allocation on -- test_a_frame_in_which_no_lane_sums
    would see a -0.0 word turn into +0.0 -- or whatever an earlier launch left)."""
    n0, n1 = 65, 300
    o = OracleWorld(512, DEPTH, FLAT); model = sc.flock_model(512); ido = sc.build_flock(o, model=model)
    g = bg.World(512, max_depth=DEPTH); ids = sc.build_flock(g)
    for w, wi in ((o, ido), (g, ids)): sc.spawn_flock(w, wi, n0, fuse_base=200, fuse_mod=1); w.set_depth(DEPTH)
    g.set_synctest_check_distance(-1)
    a = lambda f: bg.AdvanceFrame(((f * 5 + 2) & 15,), dt_bits=rd.DT_BITS)      # noqa: E731

    def both(reqs):
        want = rd.run_model(o, model, reqs)
        got = list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], g.handle_requests(reqs)))
        assert got == want, (reqs, got, want)
        assert sc.read_resources(g) == model.words(), reqs
    both([bg.SaveGameState(0), a(0)])
    small = model.words()
    assert int(g.kernel_info()["slots_covered"]) == n0
    for w, (Pos, Fz) in ((o, ido), (g, ids)):
        x, y = sc.flock_xy(1000, n1)
        w.spawn(n1, {Pos: [x.view(U32), y.view(U32)], Fz: [np.full(n1, 200, dtype=U32)]})
    both([bg.SaveGameState(1), a(1)])
    assert model.cur[2][0] == n0 + n1 and int(g.kernel_info()["slots_covered"]) == n0 + n1
    stale = sc.sum_partials(g, 0, 6)
    assert all(int(v) & 0xFFFFFFFF not in (0, sc.NEG_ZERO_32) for v in stale[2:6]), stale       # the larger launch stored real values there
    both([bg.LoadGameState(0), a(0)])
    assert model.words() == small                                                               # the same frame, the same input: the same bits
    for f in range(1, 5): both([bg.SaveGameState(f), a(f)])
    assert model.cur[2][0] == n0 and int(g.kernel_info()["slots_covered"]) == n0


def test_knob_specialised_copies_forced_at_first_sight(monkeypatch):
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    n, cd = 257, 2
    g, ids, cks, _, per_list = _gpu_session(n, cd, TICKS, before=lambda w: w._lib.ggrs_dbg_set_spec_shapes(w._p, 4))
    assert g.kernel_info()["specialised_kernel"].startswith("ready"), g.kernel_info()["specialised_kernel"]
    _compare(g, ids, cks, per_list, _reference(n, cd, TICKS), "specialised copies", cd)


def test_knob_value_tags_on():
    """Value tags stay available to such a world (k_apply_sums touches header cells only): forced on here."""
    n, cd = 257, 2
    g, ids, cks, _, per_list = _gpu_session(n, cd, TICKS, before=lambda w: w._lib.ggrs_dbg_set_value_tags(w._p, 1))
    assert g.kernel_info()["value_tags"].startswith("on"), g.kernel_info()["value_tags"]
    _compare(g, ids, cks, per_list, _reference(n, cd, TICKS), "value tags", cd)


def test_host_resource_write_of_a_summed_word_between_lists_with_rollbacks_around_it():
    """resource_write of Energy (never reset) between lists: a rollback to a frame before the edit restores the older value, one to a frame after it keeps the edit and
    the sums go on top of it.  The model receives the same edit."""
    n = 257
    o = OracleWorld(n + 128, DEPTH, FLAT); model = sc.flock_model(n + 128); _setup(o, n, model)
    g = bg.World(n + 128, max_depth=DEPTH); _setup(g, n)
    g.set_synctest_check_distance(-1)
    a = lambda f: bg.AdvanceFrame(((f * 5 + 2) & 15,), dt_bits=rd.DT_BITS)      # noqa: E731

    def both(reqs):
        want = rd.run_model(o, model, reqs)
        got = list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], g.handle_requests(reqs)))
        assert got == want, (reqs, got, want)
        assert sc.read_resources(g) == model.words(), reqs

    def edit(energy):
        g.resource_write(1, [sc.f64_bits(energy)])
        model.cur[1][0] = sc.f64_bits(energy)
        assert sc.read_resources(g) == model.words()
    for f in range(3): both([bg.SaveGameState(f), a(f)])
    before = sc.bits_f64(model.cur[1][0])
    edit(-1.0e12)                                                                                # at frame 3, before its Save
    for f in range(3, 5): both([bg.SaveGameState(f), a(f)])
    assert -1.0e12 < sc.bits_f64(model.cur[1][0]) < 0
    both([bg.LoadGameState(4), a(4), bg.SaveGameState(5), a(5)])                                 # a frame after the edit: kept
    assert -1.0e12 < sc.bits_f64(model.cur[1][0]) < 0
    both([bg.LoadGameState(2), a(2), bg.SaveGameState(3), a(3), bg.SaveGameState(4), a(4)])      # a frame before it: the older value is back, the edit is gone
    assert sc.bits_f64(model.cur[1][0]) > before > 0


def test_a_frame_costs_at_most_one_launch_more_than_without_the_sum_bindings():
    n, frames = 257, 6
    counts = {}
    for variant in ("sums", "plain"):
        g = bg.World(n + 128, max_depth=DEPTH); ids = sc.build_flock(g, variant=variant)
        sc.spawn_flock(g, ids, n); g.set_depth(DEPTH)
        g.set_synctest_check_distance(-1)
        g.handle_requests([bg.SaveGameState(0), bg.AdvanceFrame((1,), dt_bits=rd.DT_BITS)])
        g.host_timeline(1)
        for f in range(1, 1 + frames): g.handle_requests([bg.SaveGameState(f), bg.AdvanceFrame(((f + 1) & 15,), dt_bits=rd.DT_BITS)])
        counts[variant] = g.host_timeline(0)["launches"]
    assert counts["plain"] > 0 and counts["plain"] < counts["sums"] <= counts["plain"] + frames, counts


def _fanout_rank(q, lib_path):
    try:
        import os
        os.environ["GGRS_RCCL_LIB"] = lib_path
        import branch_marks_common as bm
        from bevy_ggrs_amd.fanout import RcclFanout
        n, depth, B, T, F = 257, 8, 4, 3, 3
        g = bg.World(n + 128, max_depth=depth); o = OracleWorld(n + 128, depth, FLAT); model = sc.flock_model(n + 128)
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
        res_end = sc.read_resources(g)
        native.close()
        q.put(("ok", rcode, msg, ns, listed, want, same, res_end, confirmed))
    except Exception as e:                                    # noqa: BLE001
        import traceback
        q.put(("error", f"{type(e).__name__}: {e}", traceback.format_exc()))


def test_fanout_step_works_and_branch_steps_are_refused():
    """ggrs_hip_fanout_step_branches is refused with a message; ggrs_hip_fanout_step's list form -- 4 branches x 3 frames with different inputs off one confirmed frame,
    each frame its own launch and fold -- equals the oracle's walk with the model; afterwards the live world's resources are the confirmed frame's."""
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
    _, rcode, msg, ns, listed, want, same, res_end, confirmed = r
    assert rcode == bg.GGRS_E_INVALID and "ggrs_hip_fanout_step_branches" in msg and "sum bindings" in msg and "ggrs_hip_fanout_step" in msg, (rcode, msg)
    assert ns == 1 + 4 * 3 and listed == want, (ns, listed, want)
    assert len({tuple(listed[1 + 3 * b: 4 + 3 * b]) for b in range(4)}) == 4                     # the branches diverge
    assert same and res_end == confirmed, (same, res_end, confirmed)
