"""The edges of device-decided spawns (e.spawn(n), GGRS_SPAWN_PAYLOAD_PARENT), scripted: the script world (tests/device_spawn_script.py), whose entities carry
their own trigger frame and child count in data, in BOTH forms (GGRS_TICK_JIT=1 resident, =2 streamed) against the oracle -- every Save's Checksum(u128), frame and
len after every list, the whole state where the script asks and at the end.

  * len edges: a starting len of 1, 63, 64, 65, 255, 256, 257, 511, 512, 513 (the wave edge, the 256-slot tile edge: at 256 and 512 every child lands in a tile without a
    live slot) with one parent at slot 0 and one at slot len - 1 and 1, 2 or 255 children -- (cur_len - 1) >> 8, the tiles above it, the child's binary search;
  * wide fans: three parents of one tile with 255 children each (the children span whole tiles that hold no parent); parents at slots 0, 300 and 700 with tiles
    between them that count zero (equal inclusive prefixes under the binary search) and children that straddle tile edges;
  * capacity: len + total == capacity succeeds with len == capacity, for a capacity that is a multiple of 256 and one that is not; with one slot fewer the list -- whose
    only AdvanceFrame it is -- ends in GGRS_E_CAPACITY, no child of that frame exists, and the next list is bit-equal;
  * chains: every step of a SyncTest-shaped list spawns and step s's children spawn in step s + 1, at the group's step cap and at one more step (the group is cut);
  * 22 launches that all spawn: the epochs start over on every world's 9th launch, twice in this session, with spawning launches on both sides;
  * the record: exactly 8 bindings of 4, 8, 2 and 1 bytes with narrow words left above their width; 3 bindings (tail zero); two systems calling for one entity (the
    later non-zero call wins with ITS record, a later e.spawn(0) does not replace); e.spawn(-3) gives none, e.spawn(1000) gives 255.
Every one of these comparisons fails against a deliberately wrong restatement of the oracle's callbacks: test_fuzz_device_spawn.py shows it, script by script."""
import pytest

import bevy_ggrs_amd as bg
import device_spawn_script as ds
from oracle.binding import FLAT, OracleWorld

pytestmark = pytest.mark.gpu
FORM = {"1": "one cooperative launch per request group", "2": "one streamed launch per request group"}
_WANT = {}


@pytest.fixture(params=["1", "2"], ids=["resident", "streamed"])
def form(request, monkeypatch):
    monkeypatch.setenv("GGRS_TICK_JIT", request.param)
    return request.param


def _want(name):
    """The oracle's answer to a script, computed once and shared by both forms."""
    if name not in _WANT:
        sc = ds.SCRIPTS[name][0]()
        w = OracleWorld(sc.capacity, sc.max_depth, FLAT)
        try: _WANT[name] = ds.play(w, sc)
        finally: w.close()
    return _WANT[name]


def _lens(out): return [x[2] for x in out if isinstance(x, tuple)]


def _run(name, form):
    sc = ds.SCRIPTS[name][0]()
    w = bg.World(sc.capacity, max_depth=sc.max_depth)
    try:
        got = ds.play(w, sc)
        info = w.kernel_info()
    finally: w.close()
    assert info["device_spawn"].startswith(FORM[form]), info["device_spawn"]
    want = _want(name)
    assert len(got) == len(want)
    for k, (g, o) in enumerate(zip(got, want)):
        if isinstance(g, tuple): assert g == o, f"{name}: step {k} (checksums, frame, len) differ:\n{g}\n{o}"
        else:
            bad = [key for key in o if g[key] != o[key]]
            assert not bad, f"{name}: state at step {k} differs in {bad}: len {g['len']} vs {o['len']}"
    assert want[-1]["len"] > sc.n                                                # something spawned
    return sc, got, info


@pytest.mark.parametrize("c", ds.COUNTS)
@pytest.mark.parametrize("n", ds.LENS)
def test_parents_at_slot_0_and_at_the_last_slot(n, c, form):
    sc, got, _ = _run(f"len{n}x{c}", form)
    c2 = ds.COUNTS[(ds.COUNTS.index(c) + 1) % 3] if n > 1 else 0
    assert _lens(got) == [n + c + c2 + c] * 2                                    # frame 1: c and c2 children; frame 2: the first parent's children spawn one each


def test_three_parents_of_one_tile_with_255_children_each(form):
    assert _lens(_run("three_fans", form)[1]) == [300 + 3 * 255]


def test_parents_with_empty_tiles_between_them_and_children_across_tile_edges(form):
    assert _lens(_run("fans_across", form)[1]) == [720 + 555 + 262] * 2


@pytest.mark.parametrize("capacity", [512, 519])
def test_an_exact_fit_succeeds(capacity, form):
    sc, got, _ = _run(f"fit{capacity}", form)
    assert sc.capacity == capacity and _lens(got) == [capacity - 312, capacity, capacity]


@pytest.mark.parametrize("capacity", [512, 519])
def test_one_slot_fewer_is_reported_and_the_frame_spawns_nothing(capacity, form):
    """The list that overflows holds that AdvanceFrame alone (the overflow is the launch's last step); afterwards state and len are the oracle's -- no child of that
    frame exists -- and the next list, whose frame spawns 3, is bit-equal."""
    sc, got, _ = _run(f"short{capacity}", form)
    assert sc.capacity == capacity - 1 and _lens(got) == [capacity - 312, capacity - 312, capacity - 309]


@pytest.mark.parametrize("steps", [ds.CHAIN_DEPTH + 2, ds.CHAIN_DEPTH + 3])
def test_children_that_spawn_in_the_next_step_of_the_same_list(steps, form):
    sc, got, info = _run(f"chain{steps}", form)
    assert info["group_caps"] == f"{ds.CHAIN_DEPTH + 1} saves / {ds.CHAIN_DEPTH + 2} steps", info["group_caps"]      # 6 steps: one group; 7: the group is cut
    assert _lens(got) == [5, 5 + 3 * (2 ** steps - 1), 5 + 3 * (2 ** (steps + 2) - 1)]


def test_22_launches_that_all_spawn(form):
    lens = _lens(_run("launches", form)[1])
    assert len(lens) == 23 and all(b > a for a, b in zip([64] + lens[:21], lens[:22]))


def test_a_list_of_saves_alone_leaves_len_as_the_host_knows_it(form):
    """Regression: the world's first list is [Save] -- len read 0 afterwards --, and a [Save] behind a host-side spawn -- len forgot the spawn: a launch that does not
    write the live world does not write the pinned len either, and the host took it from there all the same."""
    assert _lens(_run("saves_alone", form)[1]) == [70, 74, 79, 79, 79 + 8 + 16]


@pytest.mark.parametrize("name", ["record8", "record3"])
def test_the_record_is_the_callers_bound_words_as_the_call_left_them(name, form):
    _run(name, form)


def test_the_later_non_zero_call_wins_with_its_record(form):
    assert _lens(_run("two_callers", form)[1]) == [70 + 2 + 3 + 4 + 2 + 5]


def test_the_count_is_clamped_to_0_and_255(form):
    assert _lens(_run("clamps", form)[1]) == [70 + 255 + 255]
