"""World.query_sorted under the request fuzzers: the witness of tests/sorted_query_witness.py looks on while the HIP library runs the committed sessions against
the oracle -- 4 each of particles, generic, skirmish and the colony in its streamed form -- and holds the call, ordered by the worlds' own columns (an f32 position
word ascending; the u64 Ttl descending with a position as second key; a key on the toggled component), to sorted_query_common.model_query_sorted over the ORACLE's
states: on every held frame before the sweep (the oracle after LoadGameState(f) is frame f) and on LIVE in mid-session, once with max_rows = len + 64 and once cut
at min(TRUNC, len // 2).  Every answer is taken in both forms -- by size, and the radix launches forced -- and the two must be the same bytes.

What moves under the calls here and in no scripted session: frames saved twice, Loads in mid-list, lists in flight with host edits behind them, presence masks
rebuilt on the device (skirmish), a header len only the device knows (colony).

Every session must hit exactly the classes sorted_query_witness.HIT pins for it; test_fuzz_sorted_query.py computes those on the CPU from the oracle alone and
holds them to its coverage floors, so that this tier cannot go hollow."""
import time

import pytest

import bevy_ggrs_amd as bg
import sorted_query_witness as sw

pytestmark = pytest.mark.gpu


def _world(sc): return bg.World(sc.capacity, max_depth=8)


def _run(family, seed, on_end=None):
    w = sw.SortedWitness()
    t0 = time.perf_counter()
    log = sw.run_case(family, seed, _world, w, on_end=on_end)
    print(f"{log[0]} -- {w.asked} sorted queries, {w.sync_lists} lists looked at, classes {sw.letters(w.hit)}, {time.perf_counter() - t0:.2f} s")
    assert w.sweeps == 2 and w.sync_lists >= 1 and w.asked > 20, (w.sweeps, w.sync_lists, w.asked)
    assert sw.letters(w.hit) == sw.HIT[family, seed], (log[0], sw.letters(w.hit), sw.HIT[family, seed])      # the device session showed what the CPU tier said this seed would


def _cases(*families): return [pytest.param(f, s, id=f"{f}-{s}") for f in families for s in sw.CASES[f]]


@pytest.mark.parametrize("family,seed", _cases("particles", "generic", "skirmish"))
def test_sorted_queries_match_the_model_over_the_oracle(family, seed):
    _run(family, seed)


@pytest.mark.parametrize("family,seed", _cases("colony"))
def test_sorted_queries_match_the_model_over_the_oracle_colony_streamed(family, seed, monkeypatch):
    """Device-decided spawns, one streamed launch per request group: len is the header's, on every frame."""
    monkeypatch.setenv("GGRS_TICK_JIT", "2")

    def on_end(A, B, log):
        info = B.kernel_info()
        assert info["request_group_kernel"].startswith("ggrs_jit_tick") and info["device_spawn"].startswith("one streamed launch per request group"), info
    _run(family, seed, on_end=on_end)
