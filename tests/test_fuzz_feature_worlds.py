"""CPU tier of the feature-world fuzzer (tests/fuzz_feature_worlds.py), so that the GPU tier (test_gpu_zfuzz_feature_worlds.py) cannot go hollow.

  * the generator guard: on exactly the GPU tier's seeds and keywords the oracle adapter in its two storage modes (FLAT columns against reference-shaped per-entity
    snapshots, the second behind enqueue / collect: the stream the HIP backend gets) -- every list is accepted, every checksum, state, resource word and ring frame
    agrees.  The oracle keeps Strategies in its FLAT mode only: the strategy family's pair is FLAT twice and pins the generator alone;
  * coverage floors per family over the committed seeds -- conditions, not measurements: the list shapes a Strategy's Load and Save can be elided in, deferring
    groups and reads of owed frames on the deferral-forced seeds, the list shapes the tier exists for, and the events of each family;
  * sensitivity: every deliberately WRONG restatement of fuzz_feature_worlds.WRONG, as backend B against the right oracle, makes fuzz_util.run raise in 3/4 of the
    family's seeds with n >= 64 at least;
  * the sha256 of two logs per family, beside test_fuzz_requests.STREAMS: a later change of the generator shows.
Every count is printed before it is asserted.  A family that misses a floor gets other seeds or a sharper scenario, never a lower floor."""
import pytest

import branch_worlds_common as bw
import fuzz_feature_worlds as ff
import fuzz_user_worlds as fu
import fuzz_util

CASES = [(f, s) for f in ff.FAMILIES for s in ff.SEEDS[f]]
_SESSIONS, _WRONG = {}, {}


def _session(family, seed):
    """One committed case on the adapter pair, run once and shared: the guard is that it runs through; the floors are counted from what it returns."""
    if (family, seed) not in _SESSIONS: _SESSIONS[family, seed] = ff.cpu_pair(family, seed)
    return _SESSIONS[family, seed]


def _raises(family, seed, wrong):
    """Does fuzz_util.run notice backend B = the wrong restatement `wrong`?  Run once and shared."""
    if (family, seed, wrong) not in _WRONG:
        try: ff.cpu_pair(family, seed, wrong=wrong); _WRONG[family, seed, wrong] = False
        except AssertionError: _WRONG[family, seed, wrong] = True
    return _WRONG[family, seed, wrong]


def _big(family): return [s for s in ff.SEEDS[family] if _session(family, s)["n"] >= 64]


@pytest.mark.parametrize("family,seed", CASES, ids=[f"{f}-{s}" for f, s in CASES])
def test_oracle_modes_agree_on_random_request_lists_feature_worlds(family, seed):
    assert fu.advances(_session(family, seed)["log"]) > 0


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_the_gpu_tier_runs_24_default_seeds_and_draws_its_other_modes_from_them(family):
    """The guard above therefore covers every stream the GPU tier sees (the layout-tile session has a test of its own)."""
    seeds = ff.SEEDS[family]
    assert len(seeds) == len(set(seeds)) == 24 and ff.RUN_KW == {"n_lists": 20, "ring_sweep": True}
    for group, k in ((ff.TAGGED, 8), (ff.DEFER, 8), (ff.SPEC, 4), (ff.FOLD, 4)):
        assert len(group[family]) == len(set(group[family])) == k and set(group[family]) <= set(seeds), (family, group[family])
    sizes = {_session(family, s)["n"] for s in seeds}
    assert sizes <= set(ff.SIZES) and len(_big(family)) >= len(seeds) // 2 and {1, 2, 63} & sizes, (family, sorted(sizes))


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_the_pinned_sessions_across_the_layout_tile_hold_a_branch_list_and_a_mid_list_load(family):
    seed, n, n_lists = ff.TILE[family]
    log = ff.cpu_pair(family, seed, n=n, n_lists=n_lists)["log"]
    mid, _, branch = fu.shapes(log)
    print(f"{family}: {log[0]} -- {fu.advances(log)} AdvanceFrames, {mid} lists with a mid-list Load, {branch} branch-shaped")
    assert 8192 < n < 8192 + 256 and 0 < fu.advances(log) <= 40 and mid >= 1 and branch >= 1, (log[0], fu.advances(log), mid, branch)


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_the_logs_hold_a_load_followed_by_a_save_and_a_save_loaded_again_in_its_list(family):
    """In 3/4 of the seeds at least the log holds both a Load directly followed by a Save -- whatever is saved there must be store(load(stored)), not the slot's
    bytes -- and a Save of frame f with a later Load of f in the same list: the Load whose row versions say "identical"."""
    recs = [_session(family, s) for s in ff.SEEDS[family]]
    counts = [ff.pairs(r["log"]) for r in recs]
    met = sum(ls >= 1 and sl >= 1 for ls, sl in counts)
    print(f"{family}: {len(recs)} seeds: a Load->Save pair and a Save-f .. Load-f pair in {met}; the lowest counts {min(c[0] for c in counts)} / {min(c[1] for c in counts)}, "
          f"in all {sum(c[0] for c in counts)} / {sum(c[1] for c in counts)}")
    assert 4 * met >= 3 * len(recs), (family, met)


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_the_forced_deferral_seeds_defer_and_read(family):
    """fuzz_util.deferral_model counts one deferring group AND one read of an owed frame in 3/4 of the deferral-forced seeds at least -- a property of the streams
    alone.  (The strategy world must not defer; its streams are held to the same floor, so that the gate is tested where deferral would have happened.)"""
    res = [fuzz_util.deferral_model(_session(family, s)["log"], _session(family, s)["sc"].depth) for s in ff.DEFER[family]]
    met = sum(g >= 1 and r >= 1 for g, r in res)
    print(f"{family}: deferral-forced seeds {tuple(ff.DEFER[family])}: the model counts a deferring group and a read in {met}/{len(res)} ((groups, reads) per seed: {res})")
    assert 4 * met >= 3 * len(res), (family, res)


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_the_logs_hold_the_list_shapes_this_tier_exists_for(family):
    """test_fuzz_user_worlds.test_the_logs_hold_the_list_shapes_this_tier_exists_for, as it is: over a family's seeds ten lists at least that were enqueued and saw
    a host edit behind them before they were collected, ten with a Load that is not the first request, ten in which one frame is advanced twice."""
    recs = [_session(family, s) for s in ff.SEEDS[family]]
    edited = sum(r["edited_in_flight"] for r in recs)
    mid, twice, branch = (sum(x) for x in zip(*(fu.shapes(r["log"]) for r in recs)))
    adv = [fu.advances(r["log"]) for r in recs]
    print(f"{family}: {len(recs)} seeds, {min(adv)}..{max(adv)} AdvanceFrames per session: {edited} lists edited in flight, {mid} with a mid-list Load, "
          f"{twice} advance a frame twice, {branch} branch-shaped")
    assert edited >= 10 and mid >= 10 and twice >= 10, (family, edited, mid, twice)


# ---- the events of each family: each at least once in 3/4 of the seeds with n >= 64 -----------------------------------------------------------------------------
EVENTS = {
    "strategy": {"an entity ends with loads >= 2": lambda r: r["end"]["max_loads"] >= 2,
                 "the checksums differ from the world built without the strategies": lambda r: _raises("strategy", r["sc"].seed, "plain")},
    "inputs": {"an entity saw all three InputStatus values": lambda r: all(v >= 1 for v in r["stats"]["status"]),
               "a frame was advanced again with other bytes": lambda r: r["A"].readvanced() >= 1},
    "bullets": {"children were spawned": lambda r: r["stats"].get("children", 0) >= 1, "entities were despawned": lambda r: r["stats"].get("despawned", 0) >= 1,
                "a frame was advanced both with and without shots": lambda r: r["A"].with_and_without() >= 1},
    "clock": {"a resource write behind a list in flight": lambda r: r["res_in_flight"] >= 1,
              "a Load restored other resource words than the current ones": lambda r: r["A"].model.restored_other >= 1},
}


@pytest.mark.parametrize("family", list(EVENTS))
def test_events_of_the_family(family):
    recs = [_session(family, s) for s in _big(family)]
    for name, happened in EVENTS[family].items():
        met = sum(bool(happened(r)) for r in recs)
        print(f"{family}: {name}: in {met} of the {len(recs)} seeds with n >= 64")
        assert 4 * met >= 3 * len(recs), (family, name, met, len(recs))


def test_the_inputs_family_draws_every_layout_and_an_advance_without_inputs():
    recs = [_session("inputs", s) for s in ff.SEEDS["inputs"]]
    layouts = {(r["sc"].ib, r["sc"].players) for r in recs}
    status, const = sum(r["sc"].with_status for r in recs), sum(r["sc"].const for r in recs)
    none = sum(any(len(k[0]) == 0 for keys in r["A"].passes.values() for k in keys) for r in recs)
    print(f"inputs: layouts {sorted(layouts)}, InputStatus carried by {status}/{len(recs)} seeds, const in {const}, an AdvanceFrame with n_inputs == 0 in {none}")
    assert layouts == set(bw.LAYOUTS) and 3 * status == 2 * len(recs) and none >= 1, (sorted(layouts), status, none)


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,wrong", [(f, w) for f in ff.FAMILIES for w in ff.WRONG[f]], ids=[f"{f}-{w}" for f in ff.FAMILIES for w in ff.WRONG[f]])
def test_a_wrong_restatement_is_noticed(family, wrong):
    """The deliberately wrong restatement as backend B against the right oracle: fuzz_util.run raises in 3/4 of the family's seeds with n >= 64 at least."""
    big = _big(family)
    caught = [s for s in big if _raises(family, s, wrong)]
    print(f"{family}: `{wrong}` is noticed in {len(caught)} of the {len(big)} seeds with n >= 64 (escaped: {[s for s in big if s not in caught]})")
    assert 4 * len(caught) >= 3 * len(big), (family, wrong, len(caught), len(big))


# sha256("\n".join(log))[:16] of the committed sessions below (backend B behind enqueue / collect: the stream the HIP backend gets)
STREAMS = {("strategy", 1): "82e12d5c7465529f", ("strategy", 5): "8ac9ef161f199c57", ("inputs", 3): "4984f6bdab8b40ee", ("inputs", 14): "8733183f82c02219",
           ("bullets", 1): "5995a8aad321aff3", ("bullets", 5): "756ba72b8ee2d39d", ("hasher", 1): "56605968a090144b", ("hasher", 5): "d44a626eaf5539c6",
           ("clock", 3): "6eb59d8af33aae8a", ("clock", 7): "1f889b5f275ba61d"}


@pytest.mark.parametrize("family,seed", list(STREAMS))
def test_the_streams_of_the_feature_world_seeds_did_not_move(family, seed):
    assert fu.digest(_session(family, seed)["log"]) == STREAMS[family, seed]


def test_two_streams_per_family_are_pinned():
    assert sorted(f for f, _ in STREAMS) == sorted(2 * ff.FAMILIES) and all(s in ff.SEEDS[f] for f, s in STREAMS)
