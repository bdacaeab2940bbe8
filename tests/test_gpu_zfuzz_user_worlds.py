"""The skirmish world and the brand world under the request fuzzer (tests/fuzz_user_worlds.py, fuzz_util.run(scenario=...)): the HIP library against the oracle
adapter on random VALID request lists -- any order, one frame loaded and advanced many times in one list, re-advances with other inputs, Saves that evict their own
source, ConfirmedFrameCount and the depth moving, host despawns / inserts / removes / uploads / resource writes between lists and behind up to three lists in flight
(enqueue_requests / collect_checksums).  Until this file the per-frame device state these worlds keep beside the columns -- the peer view, the effect, remote and
reduce inboxes, the sum partials, the value payload and winner words, the resources in the snapshot header -- was tested on scripted sessions only.

Compared, through fuzz_util.run: every Save's Checksum(u128), frame / len / snapshot count after every list, the whole state every few lists and for every frame of
both ring sweeps, and for the skirmish the four resources' words against the model's.  After every list that is not in flight the rest state: the remote inbox all
zero, the reduce inbox at its identities, both winner-word arrays zero.  At the end the host policy (lazy live block off, deferred Saves off, one step per group)
and the apply counters, which equal the AdvanceFrames the log shows: nothing is skipped, nothing applied twice.

Sizes 1, 2, 63, 64, 65, 257, 1025 (one lane, the wave edge, the workgroup edge, five workgroups) and one pinned session per family across the 8192-slot layout tile.
test_fuzz_user_worlds.py runs the same seeds on the oracle's two storage modes and holds them to coverage floors, so that this tier cannot go hollow."""
import pytest

import bevy_ggrs_amd as bg
import fuzz_user_worlds as fu
import skirmish_common as sk
from test_gpu_remote_values import _inbox, _is_value_world, _winners                 # (names only: the readers of ggrs_dbg_remote_inbox / ggrs_dbg_value_winners)
from test_gpu_skirmish import _applies, _at_rest, _is_skirmish_world                 # (names only)

pytestmark = pytest.mark.gpu
BRAND_IDS = (0, 1, 2, 3, 4)                                                         # Hp, Target, Power, Burn, Mark: build_brand registers them first, in this order
APPLY_KEYS = (("peer", "peer_view"), ("effects", "effect_inbox"), ("remote", "remote_inbox"), ("reduces", "reduce_inbox"), ("sums", "sum_partials"))


def _world(spec_shapes=0):
    def make(sc):
        w = bg.World(sc.capacity, max_depth=8)
        if spec_shapes: w._lib.ggrs_dbg_set_spec_shapes(w._p, spec_shapes)
        return w
    return make


def _skirmish(seed, kinds=sk.ALL, family="skirmish", spec_shapes=0, **kw):
    def after_list(A, B, k, ctx): _at_rest(B, kinds, ctx)

    def on_end(A, B, log):
        n_adv = fu.advances(log)
        info = B.kernel_info()
        print(log[0], f"-- {n_adv} AdvanceFrames;", {key: _applies(info, key) for _, key in APPLY_KEYS if key in info}, info["group_caps"])
        if kinds == sk.ALL: _is_skirmish_world(B, n_adv)
        for kind, key in APPLY_KEYS:
            assert (key in info) == (kind in kinds), (sk.subset_id(kinds), key)
            if kind in kinds: assert _applies(info, key) == n_adv > 0, (key, info[key], n_adv)
        # the policy facts the per-feature suites assert: every kind with an apply launch has one step per group and no deferred Saves; the three that read or write
        # OTHER entities also keep the lazy live block off
        if kinds & {k for k, _ in APPLY_KEYS}: assert info["group_caps"].endswith("/ 1 steps") and info["deferred_saves"].startswith("off"), info
        if kinds & {"peer", "effects", "remote"}: assert info["lazy_live_block"].startswith("off"), info["lazy_live_block"]
        if spec_shapes: assert info["specialised_kernel"].startswith("ready"), info["specialised_kernel"]
    return fu.run(family, seed, _world(spec_shapes), kinds=kinds, after_list=after_list, on_end=on_end, **kw)[0]


def _brand(seed, spec_shapes=0, **kw):
    def after_list(A, B, k, ctx):
        assert not _inbox(B).any() and not _winners(B, BRAND_IDS[3]).any() and not _winners(B, BRAND_IDS[4]).any(), \
            f"something is left in the remote inbox or the winner words:\n{ctx}"

    def on_end(A, B, log):
        n_adv = fu.advances(log)
        print(log[0], f"-- {n_adv} AdvanceFrames;", B.kernel_info()["remote_inbox"].split("(")[-1])
        _is_value_world(B, BRAND_IDS, [[bg.AdvanceFrame()] * n_adv])                  # (it counts the AdvanceFrames of the lists it is given)
        info = B.kernel_info()
        if "effect_inbox" in info: assert f"({n_adv} applies so far)" in info["effect_inbox"], info["effect_inbox"]
        if spec_shapes: assert info["specialised_kernel"].startswith("ready"), info["specialised_kernel"]
    log, sc, _ = fu.run("brand", seed, _world(spec_shapes), after_list=after_list, on_end=on_end, **kw)
    assert sc.ids == BRAND_IDS
    return log


@pytest.mark.parametrize("seed", fu.SKIRMISH_SEEDS)
def test_skirmish_matches_the_oracle_and_the_model_on_random_request_lists(seed):
    _skirmish(seed)


@pytest.mark.parametrize("kinds,seed", fu.SUBSET_CASES, ids=[f"{sk.subset_id(k)}-{s}" for k, s in fu.SUBSET_CASES])
def test_skirmish_subsets_match_the_oracle_and_the_model_on_random_request_lists(kinds, seed):
    _skirmish(seed, kinds)


@pytest.mark.parametrize("seed", fu.SPAWN_SEEDS)
def test_skirmish_with_host_decided_spawns_matches_the_oracle_and_the_model_on_random_request_lists(seed):
    """An `A*` AdvanceFrame carries five children, whatever its frame; a frame re-advanced without them leaves the slots they had."""
    _skirmish(seed, family="spawn")


@pytest.mark.parametrize("seed", fu.BRAND_SEEDS)
def test_brand_matches_the_oracle_on_random_request_lists(seed):
    _brand(seed)


@pytest.mark.parametrize("family", ["skirmish", "brand"])
@pytest.mark.parametrize("seed", fu.FORCED_SEEDS)
def test_user_worlds_on_random_request_lists_every_shape_specialised(seed, family, monkeypatch):
    """A kernel specialised for every group shape at first sight: rx_inbox, rx_len / fx_len, sum_part and the value payload stay arguments of a specialised copy."""
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    if family == "skirmish": _skirmish(seed, spec_shapes=4)
    else: _brand(seed, spec_shapes=3)


@pytest.mark.parametrize("family", ["skirmish", "brand"])
@pytest.mark.parametrize("seed", fu.FORCED_SEEDS)
def test_user_worlds_on_random_request_lists_fold_forward_forced(seed, family, monkeypatch):
    """The checksum fold of every launch rides with the next one: here the next launch of the stream is a peer-view publish or an apply, not a tick."""
    monkeypatch.setenv("GGRS_FOLD_FORWARD_MIN_WGS", "0")
    if family == "skirmish": _skirmish(seed)
    else: _brand(seed)


@pytest.mark.parametrize("family", ["skirmish", "brand"])
def test_user_worlds_on_random_request_lists_across_the_layout_tile(family):
    """One pinned session per family with links, gathers and sends across the 8192-slot layout tile; short (the oracle calls Python once per entity, system and
    frame), and chosen so that it still holds a branch-shaped list and a Load in the middle of a list."""
    seed, n, n_lists = fu.TILE[family]
    log = (_skirmish(seed, n=n, n_lists=n_lists) if family == "skirmish" else _brand(seed, n=n, n_lists=n_lists))
    mid, _, branch = fu.shapes(log)
    assert f"n={n} " in log[0] and 0 < fu.advances(log) <= 30 and mid >= 1 and branch >= 1, (log[0], fu.advances(log), mid, branch)
