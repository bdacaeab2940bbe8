"""Bulk host edits under the request fuzzer on the device (tests/fuzz_scatter.py): the HIP library against the oracle on random VALID request lists, with
scatters -- all four ops, up to 256 rows, dead slots and slots without the component among them, now and then a planted bad row -- between the lists and behind
lists still in flight.  The oracle gets every edit one slot at a time (scatter_common.apply_per_slot), the device world through ONE World.scatter call.

Compared, through fuzz_util.run: every Save's Checksum(u128), frame / len / snapshot count after every list, the whole state every few lists and for every frame of
both ring sweeps; per edit the two reports, and the raw words and bits of every row that was not applied, read back from the device before and after the call.

36 sessions: 16 under the defaults, 8 with value tags and the lazy live block forced, 8 with deferred Saves forced on every eligible group, 4 whose worlds reach
across the 8192-slot layout tile.  test_fuzz_scatter.py runs the same seeds on the CPU and holds them to coverage floors, so that this tier cannot go hollow."""
import pytest

import bevy_ggrs_amd as bg
import fuzz_scatter as fs

pytestmark = pytest.mark.gpu


def _world(mode):
    def make(sc):
        w = bg.World(sc.capacity, max_depth=8)
        if mode == "tags_lazy": assert w._lib.ggrs_dbg_set_value_tags(w._p, 1) == 0 and w._lib.ggrs_dbg_set_lazy_live(w._p, 2 if sc.seed % 2 else 1) == 0
        if mode == "deferral": assert w._lib.ggrs_dbg_set_lazy_live(w._p, 3) == 0
        return w
    return make


@pytest.mark.parametrize("mode,family,seed", fs.ALL_CASES, ids=[f"{m}-{f}-{s}" for m, f, s in fs.ALL_CASES])
def test_scatter_matches_the_oracle_edited_per_slot_on_random_request_lists(mode, family, seed):
    seen = {}

    def on_end(A, B, log): seen["info"] = B.kernel_info()
    log, scn = fs.run_case(family, seed, _world(mode), on_end=on_end)
    print(log[0], scn.n_bulk, dict(scn.cov), seen["info"].get("scatter"))
    assert scn.n_bulk >= 2 and "scatter" in seen["info"], (log[0], scn.n_bulk)
    if mode == "tags_lazy": assert seen["info"]["value_tags"].startswith("on"), seen["info"]["value_tags"]
    if family.endswith("_tile"): assert scn.n >= fs.TILE_MIN, log[0]
