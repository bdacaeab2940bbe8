"""A component under a Strategy, PlayerInputs wider than a byte with InputStatus and n_inputs below the players, a user-written spawn system with a payload, a
user-written hasher and rollback resources without reduce or sum bindings under the request fuzzer (tests/fuzz_feature_worlds.py, fuzz_util.run(scenario=...)): the
HIP library against the oracle adapter on random VALID request lists -- any order, one frame loaded and advanced many times in one list, re-advances with other
inputs, Saves that evict their own source, ConfirmedFrameCount and the depth moving, host despawns / inserts / removes / uploads / resource writes between lists and
behind up to three lists in flight.  Until this file the special cases these five have on the host request path -- group_open touching the versions of a Strategy
component's columns after every Load, Stored words in ring-slot columns of their own, value tags leaving such a component out, the gate that keeps a Strategy world
from deferring Saves, the step record's inputs / status / n_inputs in the lazy-live and deferred-Save replays, a spawning Advance keeping its group off both, a
hasher in a specialised copy, resources beside the lazy live block -- were tested on scripted SyncTest-shaped sessions only.

Compared, through fuzz_util.run, bit for bit: every Save's Checksum(u128), frame / len / snapshot count after every list, the whole state every few lists and for
every frame of both ring sweeps, and for the clock world the resource words against the model's.  Per family: the default knobs; value tags and the lazy live block
forced; deferral forced (ggrs_dbg_set_lazy_live 3) with the library's counters held to fuzz_util.deferral_model -- for the strategy world the same call must leave
deferred Saves OFF and the counters at zero: the gate is what is tested there --; every group shape specialised at first sight; fold-forward forced; and one pinned
session across the 8192-slot layout tile.  Sizes 1, 2, 63, 64, 65, 257, 1025.  test_fuzz_feature_worlds.py runs the same seeds on the oracle alone and holds them to
coverage floors and to deliberately wrong restatements, so that this tier cannot go hollow."""
import pytest

import bevy_ggrs_amd as bg
import common as cm
import fuzz_feature_worlds as ff
import fuzz_user_worlds as fu
from test_fuzz_requests import _deferral_checked, _deferring_world, _tagged_world           # (names only: the world factories with the test hooks set)

pytestmark = pytest.mark.gpu


def _cases(seeds): return [(f, s) for f in ff.FAMILIES for s in seeds[f]]


def _ids(cases): return [f"{f}-{s}" for f, s in cases]


def _world(spec_shapes=0):
    def make(sc):
        w = bg.World(sc.capacity, max_depth=8)
        if spec_shapes: assert w._lib.ggrs_dbg_set_spec_shapes(w._p, spec_shapes) == 0
        return w
    return make


def _run(family, seed, make_b=None, on_end=None, **kw):
    def end(A, B, log):
        print(log[0], f"-- {fu.advances(log)} AdvanceFrames; deferred_saves: {B.kernel_info()['deferred_saves']}")
        if on_end is not None: on_end(A, B, log)
    return ff.run(family, seed, make_b or _world(), on_end=end, **kw)[0]


@pytest.mark.parametrize("family,seed", _cases(ff.SEEDS), ids=_ids(_cases(ff.SEEDS)))
def test_feature_worlds_match_the_oracle_on_random_request_lists(family, seed):
    _run(family, seed)


@pytest.mark.parametrize("family,seed", _cases(ff.TAGGED), ids=_ids(_cases(ff.TAGGED)))
def test_feature_worlds_on_random_request_lists_value_tags_and_lazy_live_block_forced(family, seed):
    """Value tags leave a Strategy component out (tag_cols) and keep every other column of the same world; the lazy live block has to stay correct beside it.
    It was not: strategy seeds 3, 9 and 15 (the odd ones: the lazy live block forced on every eligible list) and all eight deferral-forced strategy seeds below
    differed from the oracle in the first Save of the list that followed a list ending [.., Save(F), Advance].  That list had left the live block unwritten, and
    materialise_live rebuilt it from the ring slot of F -- which in a Strategy world holds store(x): the live world became Advance(load(store(x))) where the list
    had advanced x, one `loads` too many in Gen and one f16 rounding too many in Accel.y.  A world with a component under a Strategy now keeps its live block
    written (host_groups.hpp lazy_live_allowed)."""
    def on_end(A, B, log):
        if family == "strategy": assert B.kernel_info()["lazy_live_block"].startswith("off"), B.kernel_info()["lazy_live_block"]
    _run(family, seed, _tagged_world, on_end)


@pytest.mark.parametrize("family,seed", _cases(ff.DEFER), ids=_ids(_cases(ff.DEFER)))
def test_feature_worlds_on_random_request_lists_deferred_saves_forced(family, seed):
    """Every eligible group defers its Saves: the replays read inputs, InputStatus and n_inputs from the step record (inputs), run the user's hasher's world
    (hasher), the resource chain (clock) and the groups of the bullets world that hold no spawning Advance.  The counters are held to fuzz_util.deferral_model per
    seed.  A world with a component under a Strategy must NOT defer, whatever the knob says: a ring slot of such a world holds Stored words, and a replayed Save
    would have to run Strategy::store again."""
    if family != "strategy":
        make_b, on_end = _deferral_checked(_deferring_world)
        _run(family, seed, make_b, on_end)
        return

    def on_end(A, B, log):
        info = B.kernel_info()
        assert info["deferred_saves"].startswith("off"), f"a world with a component under a Strategy defers Saves: {info['deferred_saves']}\n{log[0]}"
        assert cm.deferred_counts(B) == (0, 0), info["deferred_saves"]
        assert info["lazy_live_block"].startswith("off"), info["lazy_live_block"]        # (the knob forces the lazy live block too: see the test above)
    _run(family, seed, _deferring_world, on_end)


@pytest.mark.parametrize("family,seed", _cases(ff.SPEC), ids=_ids(_cases(ff.SPEC)))
def test_feature_worlds_on_random_request_lists_every_shape_specialised(family, seed, monkeypatch):
    """A kernel specialised for every group shape at first sight: the Strategy sections, the user's hasher, the spawner and the resource chain in a specialised copy."""
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")

    def on_end(A, B, log):
        assert B.kernel_info()["specialised_kernel"].startswith("ready"), B.kernel_info()["specialised_kernel"]
    _run(family, seed, _world(3), on_end)


@pytest.mark.parametrize("family,seed", _cases(ff.FOLD), ids=_ids(_cases(ff.FOLD)))
def test_feature_worlds_on_random_request_lists_fold_forward_forced(family, seed, monkeypatch):
    """The checksum fold of every launch rides with the next one."""
    monkeypatch.setenv("GGRS_FOLD_FORWARD_MIN_WGS", "0")
    _run(family, seed)


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_feature_worlds_on_random_request_lists_across_the_layout_tile(family):
    """One pinned session per family across the 8192-slot layout tile; short (the oracle calls Python once per entity, system and frame), and chosen so that it
    still holds a branch-shaped list and a Load in the middle of a list."""
    seed, n, n_lists = ff.TILE[family]
    log = _run(family, seed, n=n, n_lists=n_lists)
    mid, _, branch = fu.shapes(log)
    assert f"n={n} " in log[0] and fu.advances(log) > 0 and mid >= 1 and branch >= 1, (log[0], fu.advances(log), mid, branch)
