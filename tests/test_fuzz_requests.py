"""Differential fuzzing of request lists (tests/fuzz_util.py).

CPU tier: the oracle's two storage modes against each other (FLAT columns vs the reference-shaped per-entity snapshots,
oracle/ggrs_oracle.cpp) -- this pins the GENERATOR (every list it emits is accepted, its ring model agrees with the backends
about the current frame) and the oracle's internal consistency.  GPU tier: the HIP library against the oracle on the same
seeds, small worlds around the wave / workgroup / layout-tile boundaries and two HBM-sized ones."""
import os

import pytest

import bevy_ggrs_amd as bg
import fuzz_util
from oracle.binding import FLAT, REFSHAPED, OracleWorld

# one-off sweeps (scripts/gpu_r04u.sh: the same seeds under every kernel-selecting knob, fresh seeds under the defaults):
# GGRS_FUZZ_SEEDS = how many seeds per test, GGRS_FUZZ_SEED0 = the first one
_N, _S0 = int(os.environ.get("GGRS_FUZZ_SEEDS", "0")), int(os.environ.get("GGRS_FUZZ_SEED0", "0"))
seeds = lambda n: range(_S0, _S0 + (_N or n))


@pytest.mark.parametrize("seed", seeds(40))
def test_oracle_modes_agree_on_random_request_lists(seed):
    fuzz_util.run(seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), lambda sc: OracleWorld(sc.capacity, 8, REFSHAPED), n_lists=24)


@pytest.mark.parametrize("seed", seeds(40))
def test_oracle_modes_agree_on_random_request_lists_generic_worlds(seed):
    fuzz_util.run(seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), lambda sc: OracleWorld(sc.capacity, 8, REFSHAPED), n_lists=24, generic=True)


@pytest.mark.parametrize("generic", [False, True], ids=["particles", "generic"])
@pytest.mark.parametrize("seed", seeds(120))
def test_oracle_matches_the_numpy_twin_on_random_request_lists(seed, generic):
    """The two INDEPENDENT restatements (C++ columns vs numpy per-entity snapshots, oracle/twin_np.py) on lists no session would
    emit: what pins the oracle while the reference's own checksums cannot be had."""
    from oracle.twin_np import TwinWorld
    fuzz_util.run(seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), lambda sc: TwinWorld(sc.capacity, 8), n_lists=20, generic=generic, max_n=1000)


@pytest.mark.parametrize("seed", seeds(60))
def test_oracle_matches_the_numpy_twin_on_random_request_lists_box_game(seed):
    from oracle.twin_np import TwinWorld
    fuzz_util.run(seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), lambda sc: TwinWorld(sc.capacity, 8), n_lists=20, box=True, max_n=5000)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", seeds(60))
def test_hip_matches_the_oracle_on_random_request_lists_box_game(seed):
    fuzz_util.run(seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), lambda sc: bg.World(sc.capacity, max_depth=8), n_lists=30, box=True)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", seeds(120))
def test_hip_matches_the_oracle_on_random_request_lists(seed):
    fuzz_util.run(seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), lambda sc: bg.World(sc.capacity, max_depth=8), n_lists=30)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(4))
def test_hip_matches_the_oracle_on_random_request_lists_hbm_sized(seed):
    fuzz_util.run(1000 + seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), lambda sc: bg.World(sc.capacity, max_depth=8), n_lists=10, big=True, state_every=10)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", seeds(160))
def test_hip_matches_the_oracle_on_random_request_lists_generic_worlds(seed):
    fuzz_util.run(seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), lambda sc: bg.World(sc.capacity, max_depth=8), n_lists=30, generic=True)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(3))
def test_hip_matches_the_oracle_on_random_request_lists_generic_worlds_hbm_sized(seed):
    fuzz_util.run(2000 + seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), lambda sc: bg.World(sc.capacity, max_depth=8), n_lists=10, big=True, state_every=10, generic=True)


def _lazy_world(sc):
    """The lazy live block forced on for every eligible list (test hook: no size or streak condition): whatever the fuzzer does between two lists --
    downloads, spawns, despawns, inserts, lists that open without a Load -- must find the live world the oracle has."""
    w = bg.World(sc.capacity, max_depth=8)
    assert w._lib.ggrs_dbg_set_lazy_live(w._p, 2) == 0
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("generic", [False, True], ids=["particles", "generic"])
@pytest.mark.parametrize("seed", seeds(60))
def test_hip_matches_the_oracle_on_random_request_lists_lazy_live_block_forced(seed, generic):
    fuzz_util.run(3000 + seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), _lazy_world, n_lists=30, generic=generic)


def _tagged_world(sc):
    """Value tags forced on (test hook: by default only worlds whose steady Save is bound by bytes keep them) AND the lazy live block forced: whatever the fuzzer
    does between two lists must take the tags of the bytes it wrote with it."""
    w = bg.World(sc.capacity, max_depth=8)
    assert w._lib.ggrs_dbg_set_value_tags(w._p, 1) == 0 and w._lib.ggrs_dbg_set_lazy_live(w._p, 2 if sc.seed % 2 else 1) == 0
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("generic", [False, True], ids=["particles", "generic"])
@pytest.mark.parametrize("seed", seeds(80))
def test_hip_matches_the_oracle_on_random_request_lists_value_tags_forced(seed, generic):
    fuzz_util.run(5000 + seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), _tagged_world, n_lists=30, generic=generic)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [13, 16, 43, 2, 29, 58, 71])
def test_hip_matches_the_oracle_on_random_request_lists_value_tags_forced_every_shape_specialised(seed, monkeypatch):
    """The same worlds with a kernel specialised for EVERY group shape at first sight (by default a shape earns one after 16 groups, built on a worker thread): the
    literals give the compiler other schedules than the generic text has.  Seeds 13, 16 and 43 differed from the oracle (profiles/r06ee) until set_lanes / store_lanes
    listed SCC among their clobbers (tests/test_generated_kernel.py has the static half); the whole file runs in this mode in profiles/r06gg."""
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    fuzz_util.run(5000 + seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), _tagged_world, n_lists=30, generic=True)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(3))
def test_hip_matches_the_oracle_on_random_request_lists_value_tags_forced_hbm_sized(seed):
    fuzz_util.run(6000 + seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), _tagged_world, n_lists=10, big=True, state_every=10)


@pytest.mark.parametrize("seed", seeds(60))
def test_restatements_agree_across_the_i32_frame_wrap(seed):
    """A session whose RollbackFrameCount passes i32::MAX while it runs (Frame = i32: the counters wrap, `GgrsSnapshots::push` decides
    "newer" wrap-aware while `confirm` compares plainly, mod.rs:147-202): the C++ oracle in both storage shapes and the numpy twin must
    agree on every checksum, on the state and on which frames the ring holds.  Worlds WITHOUT a time-dependent system only: past the
    wrap `GgrsTimePlugin::update` computes `frame.0 as u64 * 1_000_000_000` (src/time.rs:69-74), which overflows -- a panic in a debug
    build, garbage in a release build -- so what `Time<GgrsTime>` holds there is not defined by the reference and is not pinned here
    (stress_test and box_game integrate with it)."""
    from oracle.twin_np import TwinWorld
    kw = dict(n_lists=20, generic=True, max_n=1000, start_frame=2**31 - 1 - (seed * 3) % 40)
    fuzz_util.run(seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), lambda sc: TwinWorld(sc.capacity, 8), **kw)
    fuzz_util.run(seed, lambda sc: OracleWorld(sc.capacity, 8, FLAT), lambda sc: OracleWorld(sc.capacity, 8, REFSHAPED), **kw)


# ---- deferred Saves and lazy replays (csrc/host_groups.hpp materialise_slots / materialise_live) under the fuzzer ---------------------------------------------
# A deferred ring slot is DEFINED as its base advanced by recorded steps; no checksum sees a wrong replay (they come from the original launch's registers), only a
# later Load of that frame does.  So these tiers force deferral on every eligible group, sweep the ring (fuzz_util.run(ring_sweep=True)) and run the worlds
# that stay eligible for a whole session: the particles world, generic worlds without live-only state ("plain": 1- / 2- / 8-byte words, entities without some
# components, an immediately despawning Health) and box_game with Player under rollback (the one world whose kernel reads inputs and aux_bits AND may defer; the
# fuzzer re-advances a frame with other input bytes on purpose).
FAMILIES = {"particles": {}, "generic_plain": {"generic": True, "variant": {"plain": True}}, "box_player_rollback": {"box": True, "variant": {"player_rollback": True}}}
_family = lambda *names: pytest.mark.parametrize("family", names)


class InFlight:
    """An oracle world with the library's enqueue / collect pair: the fuzzer then draws the stream it draws for the HIP backend (lists in flight)."""
    def __init__(self, w): self.__dict__["_w"], self.__dict__["_q"] = w, []
    def __getattr__(self, k): return getattr(self._w, k)
    def enqueue_requests(self, reqs): self._q.append(list(self._w.handle_requests(reqs)))
    def collect_checksums(self): return self._q.pop(0)


def _flat(sc): return OracleWorld(sc.capacity, 8, FLAT)


def _deferring_world(sc):
    """Lazy live block AND deferred Saves forced on every eligible group (test hook: no size, streak or steadiness condition)."""
    w = bg.World(sc.capacity, max_depth=8)
    assert w._lib.ggrs_dbg_set_lazy_live(w._p, 3) == 0
    return w


def _deferring_tagged_world(sc):
    """The same with value tags forced on: a slot whose bytes lag its description must keep the tags of the bytes it really holds."""
    w = bg.World(sc.capacity, max_depth=8)
    assert w._lib.ggrs_dbg_set_value_tags(w._p, 1) == 0 and w._lib.ggrs_dbg_set_lazy_live(w._p, 3) == 0
    return w


def _deferral_checked(make):
    """(world factory, on_end): at the end of a run the library's counters are held against fuzz_util.deferral_model on the stream the run actually drew --
    a world that must have deferred did, a Load that must have found an owed slot materialised it.  Per seed, not in aggregate: a world that silently
    stops deferring in forced mode is a finding."""
    import re
    import common as cm
    seen = {}

    def make_b(sc): seen["sc"] = sc; return make(sc)

    def on_end(A, B, log):
        info = B.kernel_info()
        caps = re.match(r"(\d+) saves / (\d+) steps", info["group_caps"])
        groups, reads = fuzz_util.deferral_model(log, seen["sc"].depth, int(caps.group(1)), int(caps.group(2)))
        deferred, materialised = cm.deferred_counts(B)
        print(f"deferral: {log[0]}: model {groups} groups / {reads} reads, library {deferred} Saves deferred / {materialised} ring slots materialised")
        assert info["deferred_saves"].startswith("on"), f"the world left the deferring path: {info['deferred_saves']}\n{log[0]}"
        assert not groups or deferred > 0, f"the model counts {groups} groups that must defer, the library deferred nothing\n" + "\n".join(log)
        assert not reads or materialised > 0, f"the model counts {reads} Loads of an owed frame, the library materialised nothing\n" + "\n".join(log)
    return make_b, on_end


def _run_deferring(seed, family, make, **kw):
    make_b, on_end = _deferral_checked(make)
    fuzz_util.run(seed, _flat, make_b, **{"n_lists": 30, "ring_sweep": True, "on_end": on_end, **FAMILIES[family], **kw})


@pytest.mark.gpu
@_family("particles", "generic_plain", "box_player_rollback")
@pytest.mark.parametrize("seed", seeds(60))
def test_hip_matches_the_oracle_on_random_request_lists_deferred_saves_forced(seed, family):
    _run_deferring(7000 + seed, family, _deferring_world)


@pytest.mark.gpu
@_family("particles", "generic_plain", "box_player_rollback")
@pytest.mark.parametrize("seed", seeds(40))
def test_hip_matches_the_oracle_on_random_request_lists_deferred_saves_and_value_tags_forced(seed, family):
    _run_deferring(7200 + seed, family, _deferring_tagged_world)


@pytest.mark.gpu
@_family("generic_plain", "box_player_rollback")
@pytest.mark.parametrize("seed", range(10))
def test_hip_matches_the_oracle_on_random_request_lists_deferred_saves_every_shape_specialised(seed, family, monkeypatch):
    """A deferring group is a NEW group shape (Saves with a null destination, tested at run time in the specialised copy): every shape gets its own kernel at first sight."""
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    _run_deferring(7000 + seed, family, _deferring_world)


@pytest.mark.gpu
@_family("particles", "box_player_rollback")
@pytest.mark.parametrize("seed", range(10))
def test_hip_matches_the_oracle_on_random_request_lists_deferred_saves_fold_forward_forced(seed, family, monkeypatch):
    """The checksum fold of every launch rides with the next one (by default only beyond a workgroup count): a replay launch then carries the fold of the group before it."""
    monkeypatch.setenv("GGRS_FOLD_FORWARD_MIN_WGS", "0")
    _run_deferring(7000 + seed, family, _deferring_world)


HBM_SEEDS = [7302, 7307, 7319]      # of 7300..7323, ten lists each: seeds on which the model counts a deferring group AND a read in both families (pinned below)


@pytest.mark.gpu
@pytest.mark.parametrize("tags", [False, True], ids=["untagged", "tagged"])
@_family("particles", "generic_plain")
@pytest.mark.parametrize("seed", HBM_SEEDS)
def test_hip_matches_the_oracle_on_random_request_lists_deferred_saves_forced_hbm_sized(seed, family, tags):
    _run_deferring(seed, family, _deferring_tagged_world if tags else _deferring_world, n_lists=10, big=True, state_every=10)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", seeds(40))
def test_hip_matches_the_oracle_on_random_request_lists_lazy_live_block_forced_box_game_player_rollback(seed):
    """materialise_live replays its one step from recorded inputs, n_inputs and aux_bits: box_game with Player under rollback is the world that reads them and stays eligible."""
    def on_end(A, B, log):
        assert B.kernel_info()["deferred_saves"].startswith("on"), f"the world left the lazy path: {B.kernel_info()['deferred_saves']}\n{log[0]}"
    fuzz_util.run(7400 + seed, _flat, _lazy_world, n_lists=30, ring_sweep=True, on_end=on_end, **FAMILIES["box_player_rollback"])


# ---- CPU tier of the above: the reference side of the two new worlds, and the guards of the generator ------------------------------------------------------------
@_family("generic_plain", "box_player_rollback")
@pytest.mark.parametrize("seed", seeds(60))
def test_oracle_modes_agree_on_random_request_lists_deferral_families(seed, family):
    fuzz_util.run(7000 + seed, _flat, lambda sc: OracleWorld(sc.capacity, 8, REFSHAPED), n_lists=30, ring_sweep=True, **FAMILIES[family])


@_family("generic_plain", "box_player_rollback")
@pytest.mark.parametrize("seed", seeds(60))
def test_oracle_matches_the_numpy_twin_on_random_request_lists_deferral_families(seed, family):
    from oracle.twin_np import TwinWorld
    fuzz_util.run(7000 + seed, _flat, lambda sc: TwinWorld(sc.capacity, 8), n_lists=20, max_n=5000 if family.startswith("box") else 1000, ring_sweep=True, **FAMILIES[family])


# sha256("\n".join(log))[:16] of run(seed, FLAT, REFSHAPED, n_lists=30) with every keyword at its default, as the generator stood before `variant`, `ring_sweep`
# and `on_end` existed: (with InFlight around B -- the stream the HIP backend gets --, without)
STREAMS = {("particles", 13): ("0b3b1c2d4e49eb44", "3ea6474b0f5b569b"), ("particles", 3007): ("0c2ee25da520cfe8", "c1a6b50eb48589a1"),
           ("generic", 5013): ("9a6282a79ba7d51b", "25adfa4ea5e31c3f"), ("generic", 5016): ("aff0f92bc7975b2d", "f38d63730188c0c5"),
           ("generic", 5043): ("881d64fb142e2789", "9d9701d3ba2a3c94"), ("box", 21): ("231838ec53e38efb", "7d6a9d184acd2249")}


@pytest.mark.parametrize("kind,seed", list(STREAMS))
def test_the_streams_of_existing_seeds_did_not_move(kind, seed):
    """Existing seeds are regression seeds (13, 16, 43 found real defects): whatever the fuzzer gains must leave their random streams bit-identical."""
    import hashlib
    kw = {"generic": kind == "generic", "box": kind == "box"}
    got = tuple(hashlib.sha256("\n".join(fuzz_util.run(seed, _flat, mk, n_lists=30, **kw)).encode()).hexdigest()[:16]
                for mk in (lambda sc: InFlight(OracleWorld(sc.capacity, 8, REFSHAPED)), lambda sc: OracleWorld(sc.capacity, 8, REFSHAPED)))
    assert got == STREAMS[kind, seed]


def _model_on_the_hip_stream(seed, family, shape=REFSHAPED, **kw):
    """The stream as drawn for a backend with enqueue / collect, the model's verdict on it, and -- at every Load the model calls a read -- whether the oracle held the frame."""
    seen, held = {}, []

    class Watched(InFlight):
        def handle_requests(self, reqs):
            held.append([self._w.has_snapshot(q.frame) for q in reqs[:1] if isinstance(q, bg.LoadGameState)])
            return self._w.handle_requests(reqs)
        def enqueue_requests(self, reqs):
            held.append([self._w.has_snapshot(q.frame) for q in reqs[:1] if isinstance(q, bg.LoadGameState)])
            InFlight.enqueue_requests(self, reqs)

    def make_b(sc): seen["sc"] = sc; return Watched(OracleWorld(sc.capacity, 8, shape))
    log = fuzz_util.run(seed, _flat, make_b, **{"n_lists": 30, "ring_sweep": True, **FAMILIES[family], **kw})
    lists = [ln for ln, line in enumerate(log) if ln and all(fuzz_util._TOK.match(t) for t in line.replace("(enqueued)", "").replace("(sweep)", "").split())]
    assert len(lists) == len(held)
    reads_at = []
    groups, reads = fuzz_util.deferral_model(log, seen["sc"].depth, on_read=lambda ln, f: reads_at.append((ln, f)))
    for ln, f in reads_at:
        toks = log[ln].split()
        # a read that opens its list is checked against the oracle's ring as it stood before the list (one in the middle follows Saves of the same list: the model ring alone)
        if toks[0] == f"L{f}": assert held[lists.index(ln)] == [True], f"the model reads frame {f} in `{log[ln]}`, which the oracle's ring did not hold\n" + "\n".join(log[:ln + 1])
    return groups, reads


@pytest.mark.parametrize("base,n", [(7000, 60), (7200, 40)], ids=["7000-7059", "7200-7239"])
@_family("particles", "generic_plain", "box_player_rollback")
def test_the_forced_deferral_seeds_defer_and_read(family, base, n):
    """So that the GPU tier cannot go hollow: on the seeds it runs, the model must predict a deferring group in 3/4 of the seeds at least and a read of an owed frame
    in 3/4 at least -- a property of the generator alone.  And the model follows the ring: whenever it reports a read, the oracle held that frame."""
    res = [_model_on_the_hip_stream(base + s, family) for s in range(n)]
    defer, read = sum(g > 0 for g, _ in res), sum(r > 0 for _, r in res)
    print(f"{family} {base}..{base + n - 1}: the model predicts a deferring group in {defer}/{n} seeds ({sum(g for g, _ in res)} groups), a read in {read}/{n} ({sum(r for _, r in res)} reads)")
    assert 4 * defer >= 3 * n and 4 * read >= 3 * n, (family, defer, read, n)


@_family("particles", "generic_plain")
@pytest.mark.parametrize("seed", HBM_SEEDS)
def test_the_hbm_sized_forced_deferral_seeds_defer_and_read(seed, family):
    """Three sessions of ten lists per family are too few for a quota: each one must defer and read."""
    groups, reads = _model_on_the_hip_stream(seed, family, shape=FLAT, n_lists=10, big=True, state_every=10)      # (the stream is the generator's: per-entity snapshots of 700 k entities would only cost time)
    assert groups > 0 and reads > 0, (family, seed, groups, reads)
