"""The census world under the request fuzzer (tests/fuzz_peer_index.py, fuzz_util.run(scenario=...)): the HIP library against the oracle adapter on random VALID
request lists -- any order, one frame loaded and advanced many times in one list, Saves that evict their own source, ConfirmedFrameCount and the depth moving, host
despawns / inserts / removes / uploads of the key between lists and behind up to three lists in flight.  Every AdvanceWorld is a launch of its own with a peer-view
publish and an index build ahead of it.  Compared, through fuzz_util.run: every Save's Checksum(u128), frame / len / snapshot count after every list, the whole
state every few lists and for every frame of both ring sweeps.  At the end the build counter equals the AdvanceFrames the log shows that had a world to index.
24 sessions over the sizes 1 .. 1025 and one across the 8192-slot layout tile; test_fuzz_peer_index.py holds the same seeds to coverage floors on the oracle."""
import re

import pytest

import bevy_ggrs_amd as bg
import fuzz_peer_index as fp
import fuzz_user_worlds as fu

pytestmark = pytest.mark.gpu


def _session(seed, **kw):
    def on_end(A, B, log):
        info = B.kernel_info()
        m = re.search(r"\((\d+) builds, (\d+) launches so far\)", info["peer_index"])
        n_adv = fu.advances(log)
        print(log[0], f"-- {n_adv} AdvanceFrames;", info["peer_index"])
        assert m and int(m.group(1)) == n_adv > 0 and info["group_caps"].endswith("/ 1 steps"), (info["peer_index"], n_adv)
    return fp.run(seed, lambda sc: bg.World(sc.capacity, max_depth=8), on_end=on_end, **kw)[0]


@pytest.mark.parametrize("seed", fp.SEEDS)
def test_census_matches_the_oracle_on_random_request_lists(seed):
    _session(seed)


def test_census_on_random_request_lists_across_the_layout_tile():
    seed, n, n_lists = fp.TILE
    log = _session(seed, n=n, n_lists=n_lists)
    assert f"n={n} " in log[0] and fu.advances(log) > 0
