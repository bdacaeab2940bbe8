"""CPU tier of the device-spawn fuzzer (tests/fuzz_device_spawn.py) and of the scripted edges (tests/device_spawn_script.py), so that the GPU tiers
(test_gpu_zfuzz_device_spawn.py, test_gpu_device_spawn_edges.py) cannot go hollow.

  * the generator guard: on exactly the GPU tier's seeds the oracle adapter in its two storage modes (FLAT columns against reference-shaped per-entity snapshots, the
    second behind enqueue / collect: the stream the HIP backend gets) -- every list is accepted, every checksum, state and ring frame agrees;
  * requested == built: in every AdvanceFrame of every seed the children the split callbacks asked for are the child callbacks that ran -- the colony stays within its
    capacity by construction, so the GPU tier may treat GGRS_E_CAPACITY as a failure;
  * coverage floors, counted from the log and the callbacks, each >= 1 in EVERY seed with n >= 64 (smaller worlds are the stated exemption);
  * the sha256 of two logs: a later change of the generator shows;
  * every scripted edge: the oracle's two storage modes agree, the figures the script pins hold, and the comparison FAILS against a deliberately wrong restatement of
    the callbacks -- the proof that the GPU test of that name can fail."""
import pytest

import device_spawn_script as ds
import fuzz_device_spawn as fd
import fuzz_user_worlds as fu
from oracle.binding import FLAT, REFSHAPED, OracleWorld

_SESSIONS = {}


def _session(seed):
    if seed not in _SESSIONS: _SESSIONS[seed] = fd.cpu_pair(seed)
    return _SESSIONS[seed]


@pytest.mark.parametrize("seed", fd.SEEDS)
def test_oracle_modes_agree_on_random_request_lists_device_spawn(seed):
    rec = _session(seed)
    sc = rec["sc"]
    assert fu.advances(rec["log"]) > 0 and rec["counts"].frames == rec["counts_b"].frames > 0
    assert sc.capacity % 256 != 0 and sc.bound < sc.capacity < 65_536, (sc.bound, sc.capacity)      # (the resident form holds 256 slots x the resident workgroups: far more)


@pytest.mark.parametrize("seed", fd.SEEDS)
def test_the_children_asked_for_are_the_children_built_in_every_frame(seed):
    rec = _session(seed)
    for c in (rec["counts"], rec["counts_b"]):
        assert c.mismatches == 0 and c.frames > 0, (rec["log"][0], c.mismatches, c.frames)
    assert rec["len"] <= rec["sc"].bound, (rec["len"], rec["sc"].bound)


@pytest.mark.parametrize("seed", fd.SEEDS)
def test_floors_of_the_colony_seeds(seed):
    """A list with spawns in two consecutive steps of one request group (no Load and no cut at the group caps between them), a child that spawns later in the list that made it, a frame advanced twice with different
    child totals, a Load in a list that lowers len with a spawn behind it, a spawning list enqueued with a host edit behind it, a frame in which both systems called
    for one entity, an e.spawn(0), a frame whose children cross a 64-slot boundary and -- n >= 255 -- a 256-slot boundary."""
    rec = _session(seed)
    c = rec["counts"]
    floors = dict(c.floors(), spawning_edited=rec["spawning_edited"])
    if rec["n"] >= 255: floors["cross256"] = c.cross256
    print(rec["log"][0], f"-- {c.frames} AdvanceFrames, {c.children} children, len {rec['len']}, {rec['alive']} alive;", floors,
          f"later call won {c.later_won}, later e.spawn(0) kept the earlier {c.later_zero_kept}, negative counts {c.negative}")
    if rec["n"] >= 64: assert all(v >= 1 for v in floors.values()), (rec["log"][0], floors)


def test_the_committed_seeds_cover_the_sizes():
    big = [s for s in fd.SEEDS if _session(s)["n"] >= 64]
    assert len(big) >= 18 and {_session(s)["n"] for s in fd.SEEDS} >= {1, 2, 63, 64, 65, 255, 256, 257, 1025}
    assert set(fd.TAGGED_SEEDS) | set(fd.SPEC_SEEDS) <= set(big)


def test_the_pinned_session_crosses_the_layout_tile():
    seed, n, n_lists = fd.TILE
    rec = fd.cpu_pair(seed, n=n, n_lists=n_lists)
    c = rec["counts"]
    mid, twice, _ = fu.shapes(rec["log"])
    assert n < 8192 and c.cross8192 >= 1 and c.mismatches == 0 and 0 < fu.advances(rec["log"]) <= 30 and mid >= 1 and twice >= 1, (rec["log"][0], c.cross8192, mid, twice)


# sha256("\n".join(log))[:16] of two committed sessions (backend B behind enqueue / collect: the stream the HIP backend gets)
STREAMS = {0: "3a61c915b640ae09", 84: "3275b71cffbe27f3"}


@pytest.mark.parametrize("seed", list(STREAMS))
def test_the_streams_of_the_colony_seeds_did_not_move(seed):
    assert fu.digest(_session(seed)["log"]) == STREAMS[seed]


def test_the_host_never_rearms_a_lineage():
    sc = fd.ColonyScenario(0); sc.ids = (0, 1, 2, 3)
    assert (sc.words(0, 3, 50) == sc.max_gen).all() and int(sc.words(0, None, 4)[3]) == sc.max_gen


# ---- the scripted edges ------------------------------------------------------------------------------------------------------------------------------------------
def _play(name, mode=FLAT, perturb=None):
    sc = ds.SCRIPTS[name][0]()
    w = OracleWorld(sc.capacity, sc.max_depth, mode)
    try: return sc, ds.play(w, sc, perturb)
    finally: w.close()


@pytest.mark.parametrize("name", list(ds.SCRIPTS))
def test_a_scripted_edge_fails_against_a_wrong_restatement(name):
    sc, want = _play(name)
    assert _play(name, REFSHAPED)[1] == want
    assert want[-1]["len"] > sc.n                                                # something spawned
    wrong = ds.SCRIPTS[name][1]
    assert wrong in ds.PERTURBATIONS and _play(name, perturb=wrong)[1] != want, (name, wrong)


def _lens(out): return [x[2] for x in out if isinstance(x, tuple)]


def test_what_the_scripts_pin():
    assert _lens(_play("clamps")[1]) == [70 + 255 + 255]                         # -3 -> 0, 1000 -> 255; 256 -> 255, INT_MIN -> 0
    assert _lens(_play("two_callers")[1]) == [70 + 2 + 3 + 4 + 2 + 5]
    assert _lens(_play("three_fans")[1]) == [300 + 3 * 255]
    for cap in (512, 519):
        assert _lens(_play(f"fit{cap}")[1]) == [cap - 312, cap, cap]             # an exact fit: len == capacity
        assert _lens(_play(f"short{cap}")[1]) == [cap - 312, cap - 312, cap - 312 + 3]      # one slot fewer: the frame's spawns are dropped, the next frame's 3 fit
    for steps in (6, 7):                                                         # 3 children, then every child 2, every step of the list and the two behind it
        sc, out = _play(f"chain{steps}")
        assert sc.max_depth == ds.CHAIN_DEPTH and steps in (ds.CHAIN_DEPTH + 2, ds.CHAIN_DEPTH + 3)      # the group's step cap, and one more
        assert _lens(out) == [5, 5 + 3 * (2 ** steps - 1), 5 + 3 * (2 ** (steps + 2) - 1)]
    assert _lens(_play("saves_alone")[1]) == [70, 74, 79, 79, 79 + 8 + 16]       # 4 children, 5 from the host, then 4 x 2 and 8 x 2
    out = _play("launches")[1]
    assert len(_lens(out)) == 23 and all(b > a for a, b in zip([64] + _lens(out)[:21], _lens(out)[:22]))      # every one of the 22 launches spawned
