"""A world that uses every user-system binding kind at once -- peer reads, effects, own-entity commands, remote commands, resource reads, reducers and float sums in
ONE system and one frame (skirmish_common.py).  Everything goes through the C ABI and is compared as BITS: the Checksum(u128) of every SaveGameState equals the CPU
oracle's XOR the resource parts of the model beside it, every resource word after every list, the final state (alive, presence masks, every word of every present
component), and every frame the ring holds, loaded newest first, with the resources the Load restored.  After every list the remote inbox is all zeros and the reduce
inbox at its identities (ggrs_dbg_remote_inbox, ggrs_dbg_reduce_inbox).  NOT checked after every list: the effect inbox.  It has no debug reader, and this suite
adds no debug entry point, so "at identities after every list" cannot be read off the device for it; its rest state is inferred once, at the end of a session, the
way test_gpu_peer_effects.py does: idle frames in which nobody sends leave the effect columns alone.  (Between lists a word left in it would be applied by the next
frame and show in that frame's Checksum.)

The oracle sessions are the ones test_skirmish_text.py holds to the coverage floors -- an effect sent to an entity a remote command despawns in the same frame, a
doomed entity's reductions and sums, an own remove and a remote insert of one component in one frame --, computed once per shape and shared, unchanged.

Shapes: 1 slot, 64 / 65 (the wave edge), 257 (the workgroup edge), 1025 (five workgroups), 8300 (links cross the 8192-slot layout tile; 10 ticks at check distance 2
-- the oracle calls Python once per entity, system and frame)."""
import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
import reduces_common as rd
import skirmish_common as sk
import sums_common as sc
from oracle.binding import FLAT, OracleWorld
from test_gpu_remote_commands import _inbox                                        # (a name only: the reader of ggrs_dbg_remote_inbox)

pytestmark = pytest.mark.gpu
DEPTH = sk.DEPTH
TICKS = 14


def _reduce_layout(kinds):
    """The model's layout with only the REDUCED words marked: what reduces_common.inbox_is_identities checks."""
    return [(name, wb, [(init, None if kind == sc.SUM else kind) for init, kind in words]) for name, wb, words in sk.skirmish_layout(kinds)]


def _at_rest(g, kinds, ctx):
    if "remote" in kinds: assert not _inbox(g).any(), ctx
    if "reduces" in kinds: assert rd.inbox_is_identities(g, _reduce_layout(kinds)), ctx


def _gpu_world(n, cd, kinds=sk.ALL, *, with_spawn=False, before=None, **kw):
    g = bg.World(n + 128, max_depth=DEPTH)
    if before: before(g)
    ids = sk.build_skirmish(g, kinds, with_spawn=with_spawn, **kw); sk.spawn_skirmish(g, ids, n); g.set_depth(DEPTH)
    g.set_synctest_check_distance(cd)
    return g, ids


def _gpu_session(n, cd, ticks, kinds=sk.ALL, *, with_spawn=False, before=None):
    g, ids = _gpu_world(n, cd, kinds, with_spawn=with_spawn, before=before)
    cks, per_list, advances = [], [], 0
    for k, (confirmed, reqs) in enumerate(sk.session_lists(n, cd, ticks, with_spawn)):
        if confirmed is not None: g.set_confirmed(confirmed)
        cs = g.handle_requests(reqs)
        cks += list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], cs))
        advances += sum(isinstance(r, bg.AdvanceFrame) for r in reqs)
        per_list.append(sc.read_resources(g, 4))
        _at_rest(g, kinds, (sk.subset_id(kinds), n, "list", k))
    return g, ids, cks, per_list, advances


def _effect_inbox_at_rest(g, ids, ctx):
    """Inferred: with every link out of range and input 0, two more frames leave Hp and Score unchanged (a word left in the inbox would be applied by the first)."""
    n = g.len
    g.upload_word(ids[1], 0, 0, np.full(n, n + 1000, dtype=np.uint64))
    cols = lambda: [g.download_word(c, 0, 0, n).tolist() for c in (ids[3], ids[4])]      # noqa: E731
    before = cols()
    for _ in range(2): g.handle_requests([bg.AdvanceFrame((0,), dt_bits=rd.DT_BITS)])
    assert cols() == before, ctx


def _compare(g, ids, cks, per_list, ref, ctx, kinds=sk.ALL, min_ring=2):
    assert per_list == ref.per_list, (ctx, [k for k, (a, b) in enumerate(zip(per_list, ref.per_list)) if a != b][:3])       # every resource word's bits after every list
    assert len(cks) == len(ref.cks) > 0, (len(cks), len(ref.cks))
    for (fa, ca), (fb, cb) in zip(cks, ref.cks):
        assert fa == fb and ca == cb, f"{ctx}: frame {fa}: gpu {ca:#x} oracle ^ model {cb:#x}"
    cm.assert_states_equal(cm.snapshot_state(g, ids), ref.final, ctx)
    got = sk.ring_states(g, ids, resources=True)
    assert sorted(got) == sorted(ref.ring) and len(got) >= min_ring, (sorted(got), sorted(ref.ring))
    for f, (state, res) in got.items():
        cm.assert_states_equal(state, ref.ring[f], f"{ctx}: ring frame {f}")
        assert res == ref.model.words(ref.model.snaps[f]), (ctx, f, res, ref.model.words(ref.model.snaps[f]))
    _at_rest(g, kinds, (ctx, "after the ring walk"))
    if "effects" in kinds: _effect_inbox_at_rest(g, ids, ctx)


def _applies(info, key):
    return int(info[key].split("(")[-1].split()[0])


def _is_skirmish_world(g, advances):
    """The union of the seven features' host policies: one AdvanceWorld per launch, no lazy live block, no deferred Saves, value tags off (remote's and effects' rule
    wins over sums'), the generated kernel; one apply of each of the four kinds per AdvanceWorld executed, one peer-view publish ahead of it."""
    info = g.kernel_info()
    assert info["request_group_kernel"].startswith("ggrs_jit_tick"), info
    assert info["group_caps"].endswith("/ 1 steps"), info["group_caps"]
    assert info["lazy_live_block"].startswith("off") and info["deferred_saves"].startswith("off"), info
    assert info["value_tags"].startswith("off"), info["value_tags"]
    assert info["effect_inbox"].startswith("2 linear columns") and info["remote_inbox"].startswith("one u32 per slot, 2 remotely commanded components"), info
    assert " 2 reduced words" in info["reduce_inbox"] and " 3 summed words" in info["sum_partials"] and info["peer_view"].startswith("1 linear columns"), info
    assert info["device_resources"].startswith("4 resources, 28 bytes"), info["device_resources"]
    if advances is not None:
        for key in ("peer_view", "effect_inbox", "remote_inbox", "reduce_inbox", "sum_partials"): assert _applies(info, key) == advances > 0, (key, info[key], advances)
    return info


@pytest.mark.parametrize("n", [1, 64, 65, 257, 1025])
@pytest.mark.parametrize("cd", [2, 7])
def test_skirmish_synctest_against_the_oracle_and_the_model(n, cd):
    ref = sk.oracle_session(n, cd, TICKS)
    g, ids, cks, per_list, advances = _gpu_session(n, cd, TICKS)
    _is_skirmish_world(g, advances)
    _compare(g, ids, cks, per_list, ref, f"skirmish {n} cd {cd}")


def test_skirmish_synctest_with_links_across_the_layout_tile():
    n, cd, ticks = 8300, 2, 10
    ref = sk.oracle_session(n, cd, ticks)
    g, ids, cks, per_list, advances = _gpu_session(n, cd, ticks)
    _is_skirmish_world(g, advances)
    _compare(g, ids, cks, per_list, ref, f"skirmish {n} cd {cd}")
    links, i, final = sk.strike_links(n), np.arange(n), ref.final
    assert ((links < n) & ((links >> np.uint64(13)) != (i >> 13).astype(np.uint64))).any()      # a sender in one 8192-slot layout tile, its target in the other
    assert final["present5"][8192:].any() and final["present5"][:8192].any() and (~final["alive"][8192:]).any() and (~final["alive"][:8192]).any()


@pytest.mark.parametrize("kinds", sk.GPU_SUBSETS, ids=sk.subset_id)
def test_subset_matrix_against_the_oracle_and_the_model(kinds):
    n, cd, ticks = 257, 2, 10
    ref = sk.oracle_session(n, cd, ticks, kinds)
    g, ids, cks, per_list, _ = _gpu_session(n, cd, ticks, kinds)
    info = g.kernel_info()
    for kind, key in (("peer", "peer_view"), ("effects", "effect_inbox"), ("remote", "remote_inbox"), ("reduces", "reduce_inbox"), ("sums", "sum_partials")):
        assert (key in info) == (kind in kinds), (sk.subset_id(kinds), key)
    _compare(g, ids, cks, per_list, ref, f"subset {sk.subset_id(kinds)}", kinds)


def test_p2p_shaped_rollbacks_whose_inputs_change_between_prediction_and_confirmation():
    """Rollbacks of 0 to 7 frames; a re-simulated frame sees another input than its first simulation, so the Clock differs, k differs, and the striker sends OTHER
    commands and effects than the first time: a command, an effect, a partial or a reduction of the predicted frame that survived shows."""
    n, ticks = 300, 36
    lists = sk.session_lists(n, -1, ticks)
    assert {len([r for r in reqs if isinstance(r, bg.AdvanceFrame)]) - 1 for _, reqs in lists} == set(range(8))
    ref = sk.oracle_session(n, -1, ticks)
    g, ids, cks, per_list, advances = _gpu_session(n, -1, ticks)
    assert len(cks) > 100
    _is_skirmish_world(g, advances)
    _compare(g, ids, cks, per_list, ref, "p2p-shaped lists", min_ring=7)


def test_host_decided_spawns_children_are_not_hit_in_the_frame_they_appear():
    """Every fourth frame five children; every tenth link points at n + 5, the first child of the SECOND batch: what is sent to it in the frame it appears -- commands and
    effects -- is dropped (the oracle session counted them), its slot sums -0.0 in that frame, and from the next frame on it is hit, reduces and sums like everybody."""
    n, cd = 200, 2
    ref = sk.oracle_session(n, cd, TICKS, sk.ALL, True)
    g, ids, cks, per_list, advances = _gpu_session(n, cd, TICKS, with_spawn=True)
    _is_skirmish_world(g, advances)
    _compare(g, ids, cks, per_list, ref, "skirmish with spawns")
    assert ref.final["len"] >= n + 10 and ref.st.spawned_this_frame_dropped >= 1


@pytest.mark.parametrize("kinds", [sk.ALL, frozenset({"remote"}), frozenset({"remote", "effects"})], ids=sk.subset_id)
def test_specialised_copies_forced_at_first_sight(monkeypatch, kinds):
    """The specialiser rewrites the generated text token by token; rx_inbox, rx_len / fx_len and sum_part stay arguments of a specialised copy."""
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    n, cd, ticks = 257, 2, (TICKS if kinds == sk.ALL else 10)
    ref = sk.oracle_session(n, cd, ticks, kinds)
    g, ids, cks, per_list, _ = _gpu_session(n, cd, ticks, kinds, before=lambda w: w._lib.ggrs_dbg_set_spec_shapes(w._p, 4))
    assert g.kernel_info()["specialised_kernel"].startswith("ready"), g.kernel_info()["specialised_kernel"]
    _compare(g, ids, cks, per_list, ref, f"specialised copies {sk.subset_id(kinds)}", kinds)


def test_host_policy_is_the_union_and_forcing_value_tags_on_changes_nothing():
    """What the code does today: ggrs_dbg_set_value_tags(w, 1) is ACCEPTED (it returns 0: the knob only records the wish), and vtags_policy keeps the tags off for a
    world with effect or remote bindings -- kernel_info says "off" -- so the session gives the oracle's bits."""
    n, cd = 257, 2
    rcs = []
    g, ids, cks, per_list, advances = _gpu_session(n, cd, TICKS, before=lambda w: rcs.append(w._lib.ggrs_dbg_set_value_tags(w._p, 1)))
    assert rcs == [0]
    _is_skirmish_world(g, advances)
    _compare(g, ids, cks, per_list, sk.oracle_session(n, cd, TICKS), "value tags forced on")


def test_a_frame_costs_at_most_four_launches_more_than_with_a_striker_that_binds_nothing():
    """[Save(f), Advance] lists, one frame each; the comparison world keeps tick and countdown, its striker has its own bindings only.  The bound is four more per
    frame: the peer view's publish ahead of the group, and behind it k_apply_remote_effects (a world with both kinds applies them in ONE launch, the remote half of
    every unit first), k_apply_reduces and k_apply_sums."""
    n, frames = 257, 6
    counts = {}
    for bare in (False, True):
        g, ids = _gpu_world(n, -1, bare_striker=bare)
        g.handle_requests([bg.SaveGameState(0), bg.AdvanceFrame((1,), dt_bits=rd.DT_BITS)])          # (the first list: whatever a first launch does besides)
        g.host_timeline(1)
        for f in range(1, 1 + frames): g.handle_requests([bg.SaveGameState(f), bg.AdvanceFrame(((f + 1) & 15,), dt_bits=rd.DT_BITS)])
        counts[bare] = g.host_timeline(0)["launches"]
    print(counts)
    assert 0 < counts[True] < counts[False] <= counts[True] + 4 * frames, counts


def test_host_edits_between_lists_with_rollbacks_around_them():
    """resource_write of Energy (never reset), a host despawn of a target and an insert_component of Stun between lists: a rollback to a frame after the edits keeps
    them -- the dead target drops what is sent to it, the sums go on top of the written Energy, the inserted Stun counts down --, one to a frame before them brings
    the older world back.  The oracle and the model receive the same edits."""
    n = 257
    o = OracleWorld(n + 128, DEPTH, FLAT); model = sk.skirmish_model(sk.ALL, n + 128)
    ido = sk.build_skirmish(o, sk.ALL, model=model); sk.spawn_skirmish(o, ido, n); o.set_depth(DEPTH)
    g, ids = _gpu_world(n, -1)
    a = lambda f: bg.AdvanceFrame(((f * 9 + 15) & 15,), dt_bits=rd.DT_BITS)      # noqa: E731

    def both(reqs):
        want = rd.run_model(o, model, reqs)
        got = list(zip([r.frame for r in reqs if isinstance(r, bg.SaveGameState)], g.handle_requests(reqs)))
        assert got == want, (reqs, got, want)
        assert sc.read_resources(g, 4) == model.words(), reqs
        cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), str(reqs))
        _at_rest(g, sk.ALL, reqs)
    for f in range(3): both([bg.SaveGameState(f), a(f)])
    before = sc.bits_f64(model.cur[sk.ENERGY][0])
    links = sk.strike_links(n)
    alive = o.alive_mask(n)
    victim = next(int(t) for s, t in enumerate(links) if t < n and t != 0 and alive[s] and alive[int(t)])      # somebody's target, alive at frame 3
    stunned = next(s for s in range(n) if alive[s] and s != victim and not o.present_mask(ido[5], n)[s])
    # the edits, at frame 3, before its Save
    g.resource_write(sk.ENERGY, [sc.f64_bits(-1.0e12)]); model.cur[sk.ENERGY][0] = sc.f64_bits(-1.0e12)
    for w, wi in ((g, ids), (o, ido)):
        w.despawn(victim)
        w.insert_component(wi[5], stunned, np.array([3, 9], dtype=np.uint32))
    assert sc.read_resources(g, 4) == model.words()
    for f in range(3, 5): both([bg.SaveGameState(f), a(f)])
    assert -1.0e12 < sc.bits_f64(model.cur[sk.ENERGY][0]) < 0 and not o.alive_mask(n)[victim]
    both([bg.LoadGameState(4), a(4), bg.SaveGameState(5), a(5)])                                 # a frame after the edits: kept
    assert -1.0e12 < sc.bits_f64(model.cur[sk.ENERGY][0]) < 0 and not o.alive_mask(n)[victim]
    both([bg.LoadGameState(2), a(2), bg.SaveGameState(3), a(3), bg.SaveGameState(4), a(4)])      # a frame before them: the older world is back, the edits are gone
    assert sc.bits_f64(model.cur[sk.ENERGY][0]) > before > 0
