"""The STREAMED form of device-decided spawns (kernel_gen.hpp, STREAM): one ordinary launch per request group whose workgroups take their tiles by ticket and
number the children by a decoupled look-back, so a world whose systems call e.spawn(n) may be larger than what the device holds of its kernel as one resident
grid.  Seal takes it where the resident form does not fit (the worlds of the first two tests: refused with GGRS_E_CAPACITY before it existed);
GGRS_TICK_JIT=2 forces it on the scenarios of tests/test_gpu_device_spawn.py, each against the oracle, and one world runs in both forms."""
import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
from oracle.binding import FLAT, OracleWorld
from test_gpu_device_spawn import CHILD_SRC, MAX_GEN, PARENT, SPLIT_SRC, build, oracle_child, oracle_split
from test_gpu_device_spawn import test_children_beyond_the_capacity_are_reported as _beyond_capacity
from test_gpu_device_spawn import test_device_spawns_fuzzed as _fuzzed
from test_gpu_device_spawn import test_one_launch_per_tick_and_len_lives_on_the_device as _len_on_device
from test_gpu_device_spawn import test_parents_that_spawn_in_consecutive_frames as _guns
from test_gpu_device_spawn import test_splitting_cells_match_the_oracle as _splitting

pytestmark = pytest.mark.gpu


def streamed(w):
    return w.kernel_info()["device_spawn"].startswith("one streamed launch")


def test_parents_beyond_any_resident_grid():
    """Capacity 2 M: 600 k filler entities (a Tag only: the split system does not bind it), then 20 k splitting cells -- parents above slot 524 288, where no
    256-thread workgroup of a resident grid could ever sit on 256 CUs, and their children further up."""
    cap, fill, n, cd, ticks = 2_000_000, 600_000, 20_000, 3, 10
    res = []
    for w in (bg.World(cap, max_depth=cd + 2), OracleWorld(cap, cd + 2, FLAT)):
        tag = w.register_component("Tag", 1, 1)
        cell = w.register_component("Cell", 4, 4)
        w.checksum_component(cell, [0, 1, 2, 3]); w.checksum_component(tag, [0])
        binds = [(cell, 0), (cell, 1), (cell, 2), (cell, 3)]
        if isinstance(w, bg.World):
            w.add_custom_system(SPLIT_SRC, binds, iparam=(MAX_GEN,), name="split")
            w.add_spawn_system(CHILD_SRC, [cell], binds, payload_stride=PARENT, name="child")
        else:
            w.add_custom_system(oracle_split, binds, iparam=(MAX_GEN,))
            w.add_spawn_system(oracle_child, [cell], binds, payload_stride=PARENT)
        w.spawn(fill, {tag: [(np.arange(fill) % 5).astype(np.uint8)]})
        rng = np.random.default_rng(78)
        w.spawn(n, {cell: [rng.uniform(-50, 50, n).astype(np.float32).view(np.uint32), rng.uniform(-9, 9, n).astype(np.float32).view(np.uint32),
                           (2 + np.arange(n, dtype=np.uint32) % 9).astype(np.uint32), np.zeros(n, dtype=np.uint32)]})
        drv = cm.SyncTestDriver(w, cd, max_prediction=cd + 1)
        for _ in range(ticks - 4): drv.tick((0,))
        if isinstance(w, bg.World):
            assert streamed(w), w.kernel_info()
            w.profile_enable(True)
            for _ in range(4): drv.tick((0,))
            prof = w.profile_read(); w.profile_enable(False)
            assert prof["tick"][1] == 4, prof                                   # one launch per tick
        else:
            for _ in range(4): drv.tick((0,))
        res.append((list(drv.all_checksums), cm.snapshot_state(w, [cell, tag]), w.len))
    assert res[0][2] == res[1][2] and res[1][2] > fill + n, (res[0][2], res[1][2])
    assert res[0][0] == res[1][0]
    cm.assert_states_equal(res[0][1], res[1][1], "beyond the resident grid")


def test_a_million_live_cells():
    """1 M splitting cells in a 4 M world (the oracle's Python callbacks bound the ticks)."""
    n, cd, ticks = 1_000_000, 1, 3
    res = []
    for w in (bg.World(4 * n, max_depth=cd + 2), OracleWorld(4 * n, cd + 2, FLAT)):
        cell = build(w, n)
        drv = cm.SyncTestDriver(w, cd, max_prediction=cd + 1)
        for _ in range(ticks): drv.tick((0,))
        if isinstance(w, bg.World): assert streamed(w), w.kernel_info()
        res.append((list(drv.all_checksums), cm.snapshot_state(w, [cell]), w.len))
    assert res[0][2] == res[1][2] and res[1][2] > n, (res[0][2], res[1][2])
    assert res[0][0] == res[1][0]
    cm.assert_states_equal(res[0][1], res[1][1], "1 M cells")


@pytest.fixture
def forced(monkeypatch):
    monkeypatch.setenv("GGRS_TICK_JIT", "2")


def test_the_knob_selects_the_streamed_form(forced):
    w = bg.World(10_000, max_depth=4)
    build(w, 1000)
    w.synchronize()
    info = w.kernel_info()["device_spawn"]
    assert info.startswith("one streamed launch per request group: 40 workgroups take tiles by ticket"), info


@pytest.mark.parametrize("n,ticks,cd", [(2_000, 13, 4), (70_000, 9, 3)])
def test_splitting_cells_streamed(forced, n, ticks, cd):
    _splitting(n, ticks, cd)


@pytest.mark.parametrize("n,period,cd", [(3000, 1, 3), (20_000, 3, 4)])
def test_guns_streamed(forced, n, period, cd):
    _guns(n, period, cd)


@pytest.mark.parametrize("seed", [9001, 9002, 9003, 9004, 9005, 9006])
def test_fuzzed_streamed(forced, seed):
    _fuzzed(seed)


def test_children_beyond_the_capacity_streamed(forced):
    _beyond_capacity()


def test_len_on_the_device_streamed(forced):
    _len_on_device()


def test_both_forms_agree_bit_for_bit(monkeypatch):
    n, cd, ticks = 70_000, 3, 9
    res = []
    for form in ("1", "2"):
        monkeypatch.setenv("GGRS_TICK_JIT", form)
        w = bg.World(4 * n + 256, max_depth=cd + 2)
        cell = build(w, n)
        drv = cm.SyncTestDriver(w, cd, max_prediction=cd + 1)
        for _ in range(ticks): drv.tick((0,))
        assert streamed(w) == (form == "2"), w.kernel_info()
        res.append((list(drv.all_checksums), cm.snapshot_state(w, [cell]), w.len))
    assert res[0][2] == res[1][2] and res[0][2] > n
    assert res[0][0] == res[1][0]
    cm.assert_states_equal(res[0][1], res[1][1], "resident vs streamed")


def test_groups_run_in_place_streamed(forced):
    """P2P-shaped lists: many groups are [Save(F), Advance] on the live block itself, so every tile reads its starting len from the header the grid's last tile
    rewrites at the end of the launch (it waits until every tile has read it)."""
    n, ticks = 20_000, 14
    res = []
    for w in (bg.World(4 * n, max_depth=4), OracleWorld(4 * n, 4, FLAT)):
        cell = build(w, n)
        drv = cm.P2PShapeDriver(w, max_rollback=2, seed=11)
        for _ in range(ticks): drv.tick()
        if isinstance(w, bg.World): assert streamed(w), w.kernel_info()
        res.append((list(drv.all_checksums), cm.snapshot_state(w, [cell]), w.len, list(drv.depths)))
    assert res[0][3].count(0) >= 3, res[0][3]                                    # in-place groups happened
    assert res[0][2] == res[1][2] and res[0][2] > n, (res[0][2], res[1][2])
    assert res[0][0] == res[1][0]
    cm.assert_states_equal(res[0][1], res[1][1], "in place")
