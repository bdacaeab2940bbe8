"""CPU tier of the user-world fuzzer (tests/fuzz_user_worlds.py), so that the GPU tier (test_gpu_zfuzz_user_worlds.py) cannot go hollow.

  * the generator guard: on exactly the GPU tier's seeds and keywords the oracle adapter in its two storage modes (FLAT columns against reference-shaped per-entity
    snapshots, the second behind enqueue / collect: the stream the HIP backend gets) -- every list is accepted, every checksum, state, resource word and ring frame
    agrees;
  * coverage floors per family over the committed seeds -- conditions, not measurements: the cross-feature events of skirmish_common.Stats / remote_values_common.Stats
    happen, the worlds stay populated, and the logs hold the list shapes the tier exists for;
  * the sha256 of two logs per family, beside test_fuzz_requests.STREAMS: a later change of the generator shows;
  * the three hazards of the oracle callbacks that the begin_frame hook closes, each as a hand-written session that goes wrong without the hook and right with it.
Two oracles that share the same Python callbacks cannot catch a defect in those callbacks: the hazard tests compare with a FRESH world that never saw the earlier
pass."""
import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
import fuzz_user_worlds as fu
import reduces_common as rd
import remote_values_common as rv
import skirmish_common as sk
from oracle.binding import FLAT

CASES = ([("skirmish", s, sk.ALL) for s in fu.SKIRMISH_SEEDS] + [("skirmish", s, k) for k, s in fu.SUBSET_CASES] + [("spawn", s, sk.ALL) for s in fu.SPAWN_SEEDS]
         + [("brand", s, sk.ALL) for s in fu.BRAND_SEEDS])


_SESSIONS = {}


def _session(family, seed, kinds=sk.ALL):
    """One committed case on the adapter pair, run once and shared: the guard is that it runs through; the floors are counted from what it returns."""
    key = (family, seed, kinds)
    if key not in _SESSIONS: _SESSIONS[key] = fu.cpu_pair(family, seed, kinds=kinds)
    return _SESSIONS[key]


@pytest.mark.parametrize("family,seed,kinds", CASES, ids=[f"{f}-{sk.subset_id(k) if k != sk.ALL else 'all'}-{s}" for f, s, k in CASES])
def test_oracle_modes_agree_on_random_request_lists_user_worlds(family, seed, kinds):
    rec = _session(family, seed, kinds)
    assert fu.advances(rec["log"]) > 0


@pytest.mark.parametrize("family", ["skirmish", "brand"])
def test_the_pinned_sessions_across_the_layout_tile_hold_a_branch_list_and_a_mid_list_load(family):
    seed, n, n_lists = fu.TILE[family]
    log = fu.cpu_pair(family, seed, n=n, n_lists=n_lists)["log"]
    mid, _, branch = fu.shapes(log)
    assert 0 < fu.advances(log) <= 30 and mid >= 1 and branch >= 1, (log[0], fu.advances(log), mid, branch)


def _floored(recs, counters):
    """Of the sessions with 64 entities or more: how many there are, and how many meet the floor -- every counter of `counters(stats)` is above zero AND, in that same
    session, a quarter of the spawned entities is alive at the last list."""
    big = [r for r in recs if r["n"] >= 64]
    return big, sum(all(v >= 1 for v in counters(r["stats"]).values()) and 4 * r["alive"] >= r["len"] for r in big)


@pytest.mark.parametrize("family,seeds", [("skirmish", fu.SKIRMISH_SEEDS), ("spawn", fu.SPAWN_SEEDS)])
def test_floors_of_the_skirmish_seeds(family, seeds):
    """In 3/4 of the seeds with n >= 64 every cross-feature counter is above zero and, in those same seeds, a quarter of the spawned entities is alive at the last
    list; in the spawn variant something sent to an entity spawned in that frame is dropped in half of the seeds at least.  If the oracle alone misses one, the
    SCENARIO changes (fuses, links)."""
    recs = [_session(family, s) for s in seeds]
    big, met = _floored(recs, lambda st: st.cross())
    dropped = sum(r["stats"].spawned_this_frame_dropped >= 1 for r in recs)
    lows = {k: min(r["stats"].cross()[k] for r in big) for k in big[0]["stats"].cross()}
    print(f"{family}: {len(recs)} seeds, {len(big)} with n >= 64: every cross counter >= 1 and a quarter alive at the last list in {met}, "
          f"spawned_this_frame_dropped >= 1 in {dropped}/{len(recs)}; the lowest counters {lows}")
    assert len(big) >= len(recs) // 2 and 4 * met >= 3 * len(big), (family, len(big), met)
    if family == "spawn": assert 2 * dropped >= len(recs), (dropped, len(recs))


def test_floors_of_the_brand_seeds():
    """In 3/4 of the seeds with n >= 64 every floor of remote_values_common.Stats but spawned_this_frame (the fuzzed world has no spawn system) is above zero and, in
    those same seeds, a quarter of the spawned entities is alive at the last list; both applies (remote-only and fused with the effects) are drawn."""
    recs = [_session("brand", s) for s in fu.BRAND_SEEDS]
    big, met = _floored(recs, lambda st: {k: v for k, v in st.floors().items() if k != "spawned_this_frame"})
    names = [k for k in big[0]["stats"].floors() if k != "spawned_this_frame"]
    fused = sum("effects=True" in r["log"][0] for r in recs)
    print(f"brand: {len(recs)} seeds, {len(big)} with n >= 64: every floor >= 1 and a quarter alive at the last list in {met}, the fused apply in {fused}; "
          f"the lowest counters { {k: min(r['stats'].floors()[k] for r in big) for k in names} }")
    assert len(big) >= len(recs) // 2 and 4 * met >= 3 * len(big), (len(big), met)
    assert 10 <= fused <= len(recs) - 10, fused


@pytest.mark.parametrize("family,seeds", [("skirmish", fu.SKIRMISH_SEEDS), ("spawn", fu.SPAWN_SEEDS), ("brand", fu.BRAND_SEEDS)])
def test_the_logs_hold_the_list_shapes_this_tier_exists_for(family, seeds):
    """Over a family's seeds: ten lists at least that were enqueued and saw a host edit behind them before they were collected, ten with a Load that is not the first
    request, ten in which one frame is advanced twice."""
    recs = [_session(family, s) for s in seeds]
    edited = sum(r["edited_in_flight"] for r in recs)
    mid, twice, branch = (sum(x) for x in zip(*(fu.shapes(r["log"]) for r in recs)))
    adv = [fu.advances(r["log"]) for r in recs]
    print(f"{family}: {len(recs)} seeds, {min(adv)}..{max(adv)} AdvanceFrames per session: {edited} lists edited in flight, {mid} with a mid-list Load, "
          f"{twice} advance a frame twice, {branch} branch-shaped")
    assert edited >= 10 and mid >= 10 and twice >= 10, (family, edited, mid, twice)


# sha256("\n".join(log))[:16] of the committed sessions below (backend B behind enqueue / collect: the stream the HIP backend gets)
STREAMS = {("skirmish", 0): "807448608686089e", ("skirmish", 3): "c90b3e726c61aedf", ("spawn", 200): "1a806d78ab33ca31", ("spawn", 205): "38908c6bd06ef4ac",
           ("brand", 1): "f70ffc50b685094a", ("brand", 5): "eafc7e833b3443dc"}


@pytest.mark.parametrize("family,seed", list(STREAMS))
def test_the_streams_of_the_user_world_seeds_did_not_move(family, seed):
    assert fu.digest(_session(family, seed)["log"]) == STREAMS[family, seed]


# ---- the three hazards of the oracle callbacks --------------------------------------------------------------------------------------------------------------------
def _brand_pair(n, hook):
    sc = fu.BrandScenario(0, n=n); sc.effects = False
    w = sc.oracle(FLAT, hook); ids = sc.build(w); w.set_depth(4)
    return w, ids


def _skirmish_pair(n, hook):
    sc = fu.SkirmishScenario(0, n=n)
    w = sc.oracle(FLAT, hook); ids = sc.build(w); w.set_depth(4)
    return w, ids


def _state(w, ids):
    s = cm.snapshot_state(w, ids)
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in s.items()}


def test_hazard_a_second_pass_over_the_same_frame_that_starts_at_a_higher_slot():
    """`A L0 A` over frame 0, n = 2: the first pass runs for slot 0 alone (slot 1 was despawned by the host), the Load brings slot 1 back, the host despawns slot 0
    and sets slot 1 on fire, and the second pass starts at slot 1 -- above where the first ended, in the same frame.  _Pass.begin takes it for the first pass's
    continuation: the countdown reads the presence bits of the first pass and leaves the Burn alone, and torch computes nothing, so the commands of the first pass land again.  With the hook it is counted down and removed (and nobody
    brands slot 1 anew: the step sees frame 1, slot + frame = 2 sends a Mark and a default insert to slot 0, which is dead)."""
    burn = np.array([7, 1, 5], dtype=np.uint32)                                    # ticks 1: the countdown removes it

    def session(hook, fresh):
        w, ids = _brand_pair(2, hook)
        a = lambda: bg.AdvanceFrame((1,))      # noqa: E731
        if not fresh:
            w.handle_requests([bg.SaveGameState(0)]); w.despawn(1); w.handle_requests([a(), bg.LoadGameState(0)])
        w.despawn(0); w.insert_component(ids[3], 1, burn)
        w.handle_requests([a()])
        return _state(w, ids)
    want = session(True, True)
    assert want["alive"] == [False, True] and not want["present3"][1]             # the fresh world removed it
    assert session(True, False) == want
    stale = session(False, False)
    assert stale != want and stale["present3"][1]                                 # not counted down, and branded by what slot 0 sent in the FIRST pass


def test_hazard_torch_runs_for_nobody_and_nothing_is_applied():
    """n = 1: in its first step (which sees frame 1: slot + frame = 1) the lone entity brands itself -- torch's second value binding, onto (Target + 1) % n, with the
    default's 3 ticks.  Then the host removes its Power: torch runs for nobody in the next step, no command is computed, and `apply` must apply nothing -- the Burn
    counts down from 3 to 2.  Without the hook the commands of the first step are still in the record and are applied again: the Burn is re-inserted with 3 ticks."""
    def session(hook):
        w, ids = _brand_pair(1, hook)
        w.handle_requests([bg.AdvanceFrame((0,))])
        assert w.present_mask(ids[3], 1)[0] and int(w.download_word(ids[3], 1, 0, 1)[0]) == 3
        landed = w.stats.landed
        w.remove_component(ids[2], 0)
        w.handle_requests([bg.AdvanceFrame((0,))])
        return int(w.download_word(ids[3], 1, 0, 1)[0]), w.stats.landed - landed
    assert session(True) == (2, 0)
    assert session(False) == (3, 1)


def test_hazard_a_frame_advanced_again_in_which_the_striker_runs_for_nobody():
    """Skirmish, n = 1: `S0 A L0`, the host removes Pos, `A` again -- frame 0 twice, and the second time the striker runs for nobody.  The frame check of apply_remote
    and of the effect applies (sn.frame != f.frame) passes, because it IS the same frame: without the hook the effects of the first pass land on Hp and Score again."""
    def session(hook, fresh):
        w, ids = _skirmish_pair(1, hook)
        a = lambda: bg.AdvanceFrame((3,), dt_bits=rd.DT_BITS)      # noqa: E731
        if not fresh: w.handle_requests([bg.SaveGameState(0), a(), bg.LoadGameState(0)])
        w.remove_component(ids[0], 0)
        w.handle_requests([a()])
        return _state(w, ids), w.model.words()
    want = session(True, True)
    assert session(True, False) == want
    assert session(False, False) != want


@pytest.mark.parametrize("family", ["skirmish", "brand"])
def test_landing_the_applies_by_host_calls_gives_the_bits_of_the_registered_callbacks(family):
    """The adapter does not register the oracle's apply callbacks as systems (they would run only for entities that have Target) but lands them by host calls behind
    every AdvanceFrame.  Where every entity has Target -- the scripted sessions: SyncTest at check distance 2, host-decided spawns included -- the two ways must give
    the same checksums and the same state."""
    got = []
    for host_apply in (False, True):
        sc = fu.SkirmishScenario(0, with_spawn=True, n=257) if family == "skirmish" else fu.BrandScenario(1, n=257)
        w = sc.oracle(FLAT, host_apply=host_apply); ids = sc.build(w); w.set_depth(sk.DEPTH)
        lists = [reqs for _, reqs in sk.session_lists(257, 2, 12, True)] if family == "skirmish" else rv.p2p_lists()
        got.append(([w.handle_requests(reqs) for reqs in lists], _state(w, ids), w.stats.__dict__))
    assert got[0] == got[1] and sum(len(c) for c in got[0][0]) > 20
