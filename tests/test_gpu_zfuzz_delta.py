"""World.delta under the request fuzzers: the witness of tests/delta_witness.py looks on while the HIP library runs the committed sessions against the oracle, and
holds every kind of delta -- adjacent held frames, oldest against newest in both orders, LIVE against the newest, frames against snapshot_copy blocks, and the two
newest frames in mid-session -- to delta_common.model_delta over the ORACLE's states (the oracle after LoadGameState(f) is frame f).

What moves under the calls here and in no scripted session: frames saved twice, Loads in mid-list, lists in flight with host edits behind them, presence masks
rebuilt on the device (skirmish), a header len only the device knows (colony, both forms of its kernel), owed ring slots and a lazily skipped live block (deferred
Saves forced: a delta is then often the first reader of an owed slot), value tags forced, and two sessions across the 8192-slot layout tile.

Every session must hit exactly the classes delta_witness.HIT pins for it; test_fuzz_delta.py computes those on the CPU from the oracle alone, holds them to its
coverage floors and shows the wrong models caught, so that this tier cannot go hollow."""
import time

import pytest

import bevy_ggrs_amd as bg
import common as cm
import delta_witness as dw
from test_fuzz_requests import _deferring_world, _tagged_world                       # (names only: the world factories with the test hooks set)

pytestmark = pytest.mark.gpu


def _world(sc): return bg.World(sc.capacity, max_depth=8)


def _run(family, seed, make_b=_world, on_end=None):
    w = dw.DeltaWitness()
    t0 = time.perf_counter()
    log = dw.run_case(family, seed, make_b, w, on_end=on_end)
    print(f"{log[0]} -- {w.asked} delta calls, {w.sync_lists} lists looked at, classes {dw.letters(w.hit)}, {time.perf_counter() - t0:.2f} s")
    assert w.sweeps == 2 and w.sync_lists >= 1 and w.asked > 20, (w.sweeps, w.sync_lists, w.asked)
    assert dw.letters(w.hit) == dw.HIT[family, seed], (log[0], dw.letters(w.hit), dw.HIT[family, seed])      # the device session showed what the CPU tier said this seed would
    return w


FORM = {"1": "one cooperative launch per request group", "2": "one streamed launch per request group"}      # kernel_info()["device_spawn"], by GGRS_TICK_JIT


def _colony(family, seed, form, monkeypatch):
    monkeypatch.setenv("GGRS_TICK_JIT", form)

    def on_end(A, B, log):
        info = B.kernel_info()
        assert info["request_group_kernel"].startswith("ggrs_jit_tick") and info["device_spawn"].startswith(FORM[form]) and "delta" in info, info
    _run(family, seed, on_end=on_end)


def _cases(*families): return [pytest.param(f, s, id=f"{f}-{s}") for f in families for s in dw.CASES[f]]


@pytest.mark.parametrize("family,seed", _cases("particles", "generic", "box"))
def test_deltas_match_the_model_over_the_oracle(family, seed):
    _run(family, seed)


@pytest.mark.parametrize("family,seed", _cases("plain"))
def test_deltas_match_the_model_over_the_oracle_deferred_saves_forced(family, seed):
    """Lazy live block and deferred Saves forced on every eligible group: the delta calls bring owed ring slots and the live block up to date first."""
    def on_end(A, B, log): assert cm.deferred_counts(B)[0] > 0, (log[0], B.kernel_info()["deferred_saves"])
    _run(family, seed, _deferring_world, on_end=on_end)


@pytest.mark.parametrize("family,seed", _cases("tagged_particles", "tagged_generic"))
def test_deltas_match_the_model_over_the_oracle_value_tags_forced(family, seed):
    _run(family, seed, _tagged_world)


@pytest.mark.parametrize("family,seed", _cases("skirmish"))
def test_deltas_match_the_model_over_the_oracle_skirmish(family, seed):
    """Commands, remote commands and value bindings: the presence masks change on the device, between any two frames."""
    _run(family, seed)


@pytest.mark.parametrize("form", ["1", "2"], ids=["resident", "streamed"])
@pytest.mark.parametrize("family,seed", _cases("colony"))
def test_deltas_match_the_model_over_the_oracle_colony(family, seed, form, monkeypatch):
    """Device-decided spawns: both lens are the headers', n_beyond_old_len counts what the device spawned; in both forms of the kernel."""
    _colony(family, seed, form, monkeypatch)


@pytest.mark.parametrize("family,seed", _cases("skirmish_tile"))
def test_deltas_match_the_model_over_the_oracle_across_the_layout_tile(family, seed):
    """The pinned session of fuzz_user_worlds.TILE: masks, compared columns and rows on both sides of slot 8192."""
    _run(family, seed)


def test_deltas_match_the_model_over_the_oracle_colony_across_the_layout_tile(monkeypatch):
    """The pinned session of fuzz_device_spawn.TILE: the header len crosses slot 8192 between held frames."""
    _colony("colony_tile", dw.CASES["colony_tile"][0], "2", monkeypatch)
