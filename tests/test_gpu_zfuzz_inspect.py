"""The inspection calls -- World.checksum_parts, World.diff, World.query, World.snapshot_copy and their block forms -- under the request fuzzers: the witness of
tests/inspect_witness.py looks on while the HIP library runs the committed sessions of every fuzzed family against the oracle, and holds what the library says about
the live world and about every ring frame to the numpy models over the ORACLE's states (the oracle after LoadGameState(f) is frame f).  Until this file the three
calls were compared with models fed by the library's own downloads, on scripted sessions.

What moves under the calls here and in no scripted session: a frame saved twice, Saves that evict their own source, Loads in mid-list, re-advances, lists in flight
with host edits behind them, the depth and ConfirmedFrameCount moving; resource cells that flip behind apply launches (skirmish), presence masks rebuilt on the device
(commands, remote commands, value bindings: skirmish, brand), a header len only the device knows (colony, both forms), owed ring slots and a lazily skipped live block
(deferred Saves forced), value tags forced.  The calls are made in mid-session too (every sixth list on LIVE, every list on the frames near the current one): they
materialise owed slots and the live block, and the session must go on bit-equal -- fuzz_util.run's own assertions.

Every session must hit exactly the classes inspect_witness.HIT pins for it; test_fuzz_inspect.py computes those on the CPU from the oracle alone, holds them to
coverage floors and shows that the witness catches five wrong inspectors, so that this tier cannot go hollow."""
import time

import pytest

import bevy_ggrs_amd as bg
import common as cm
import inspect_witness as iw
from test_fuzz_requests import _deferring_world, _tagged_world                       # (names only: the world factories with the test hooks set)

pytestmark = pytest.mark.gpu


def _world(sc): return bg.World(sc.capacity, max_depth=8)


def _run(family, seed, make_b=_world, probe=None, on_end=None):
    w = iw.Witness(probe=probe)
    t0 = time.perf_counter()
    log = iw.run_case(family, seed, make_b, w, on_end=on_end)
    print(f"{log[0]} -- {w.asked} inspection calls, {w.sync_lists} lists looked at, classes {iw.letters(w.hit)}, {time.perf_counter() - t0:.2f} s")
    assert w.sweeps == 2 and w.sync_lists >= 1 and w.asked > 20, (w.sweeps, w.sync_lists, w.asked)
    assert iw.letters(w.hit) == iw.HIT[family, seed], (log[0], iw.letters(w.hit), iw.HIT[family, seed])      # the device session showed what the CPU tier said this seed would
    return w


FORM = {"1": "one cooperative launch per request group", "2": "one streamed launch per request group"}      # kernel_info()["device_spawn"], by GGRS_TICK_JIT


def _colony(family, seed, form, monkeypatch):
    monkeypatch.setenv("GGRS_TICK_JIT", form)

    def on_end(A, B, log):
        info = B.kernel_info()
        assert info["request_group_kernel"].startswith("ggrs_jit_tick") and info["device_spawn"].startswith(FORM[form]), info
    _run(family, seed, on_end=on_end)


def _cases(*families): return [pytest.param(f, s, id=f"{f}-{s}") for f in families for s in iw.CASES[f]]


@pytest.mark.parametrize("family,seed", _cases("particles", "generic", "box"))
def test_inspection_calls_match_the_models_over_the_oracle(family, seed):
    _run(family, seed)


@pytest.mark.parametrize("family,seed", _cases("plain"))
def test_inspection_calls_match_the_models_over_the_oracle_deferred_saves_forced(family, seed):
    """Lazy live block and deferred Saves forced on every eligible group: an inspection call is then often the FIRST reader of an owed ring slot.  The seeds are
    those on which the stream alone says that Saves must be deferred and an owed frame is read (test_fuzz_inspect.py): Saves were deferred, and the count of ring
    slots materialised on demand grew across one witness call at least."""
    def on_end(A, B, log): assert cm.deferred_counts(B)[0] > 0, (log[0], B.kernel_info()["deferred_saves"])
    w = _run(family, seed, _deferring_world, probe=lambda B: cm.deferred_counts(B)[1], on_end=on_end)
    assert w.probe_grew, "no inspection call found an owed ring slot"


@pytest.mark.parametrize("family,seed", _cases("tagged_particles", "tagged_generic"))
def test_inspection_calls_match_the_models_over_the_oracle_value_tags_forced(family, seed):
    _run(family, seed, _tagged_world)


@pytest.mark.parametrize("family,seed", _cases("skirmish", "spawn", "brand"))
def test_inspection_calls_match_the_models_over_the_oracle_user_worlds(family, seed):
    """Reduces, sums, remote commands, value bindings, peer effects: the resource cell flips behind the apply launches, the presence masks change on the device."""
    _run(family, seed)


@pytest.mark.parametrize("form", ["1", "2"], ids=["resident", "streamed"])
@pytest.mark.parametrize("family,seed", _cases("colony"))
def test_inspection_calls_match_the_models_over_the_oracle_colony(family, seed, form, monkeypatch):
    """Device-decided spawns: len is the header's, in both forms of the kernel."""
    _colony(family, seed, form, monkeypatch)


@pytest.mark.parametrize("family,seed", _cases("skirmish_tile", "brand_tile"))
def test_inspection_calls_match_the_models_over_the_oracle_across_the_layout_tile(family, seed):
    """The pinned sessions of fuzz_user_worlds.TILE: masks, columns and rows on both sides of slot 8192."""
    _run(family, seed)


@pytest.mark.parametrize("form", ["1", "2"], ids=["resident", "streamed"])
def test_inspection_calls_match_the_models_over_the_oracle_colony_across_the_layout_tile(form, monkeypatch):
    """The pinned session of fuzz_device_spawn.TILE: the header len crosses slot 8192 between held frames."""
    _colony("colony_tile", iw.CASES["colony_tile"][0], form, monkeypatch)
