"""CPU tier of the branch-step tests over wide inputs, InputStatus and Strategy (tests/branch_worlds_common.py), oracle only: what shows that the GPU tier
(test_gpu_branch_worlds.py, test_gpu_zfuzz_branch_worlds.py) could fail.

  * sensitivity: in every input layout one flipped input byte -- at each byte position of one player's input in one (branch, frame) --, one flipped InputStatus byte
    each change that branch's oracle checksums, and only that branch's; n_inputs lowered by one (a step carries one n_inputs for all its branches) changes every
    branch's: a library that packed one byte of a member's input rows wrongly could not produce the oracle's table;
  * coverage floors over the fuzz tier's exact seeds, the generator run with the oracle and no library."""
import numpy as np
import pytest

import bevy_ggrs_amd as bg
import branch_worlds_common as bw
from oracle.binding import FLAT, OracleWorld

B, T, N = 3, 2, 64


def _tables(ib, players, const, inputs, status, n_inputs):
    ow = OracleWorld(N + 8, 6, FLAT)
    bw.build_inputs(ow, N, ib, players, const, bw.new_stats())
    ow.set_depth(5)
    ow.set_confirmed(0)
    return bw.oracle_walk(ow, [bg.SaveGameState(0)], inputs, status, n_inputs, True)[2]


@pytest.mark.parametrize("ib,players", bw.LAYOUTS)
def test_one_wrong_byte_of_a_branch_frames_inputs_changes_that_branch_alone(ib, players):
    rng = np.random.default_rng([ib, players])
    inputs = rng.integers(0, 256, size=(B, T, players, ib)).astype(np.uint8)
    status = rng.integers(0, 3, size=(B, T, players)).astype(np.uint8)
    base = _tables(ib, players, False, inputs, status, players)
    assert len(base) == B and all(len(t) == T for t in base) and len({tuple(t) for t in base}) == B
    b, i, p = 1, 1, players - 1                                  # the last frame of the middle branch, the last player: the end of a member's input rows
    for pos in range(ib):
        flipped = inputs.copy(); flipped[b, i, p, pos] ^= 0x10
        got = _tables(ib, players, False, flipped, status, players)
        assert got[b][-1] != base[b][-1] and got[b][:-1] == base[b][:-1], (ib, players, "input byte", pos)
        assert all(got[k] == base[k] for k in range(B) if k != b), (ib, players, "input byte", pos, "another branch changed")
    st = status.copy(); st[b, i, p] = (st[b, i, p] + 1) % 3
    got = _tables(ib, players, False, inputs, st, players)
    assert got[b][-1] != base[b][-1] and got[b][:-1] == base[b][:-1] and all(got[k] == base[k] for k in range(B) if k != b), (ib, players, "status byte")
    # the first frame's bytes reach the first frame's Save (and what follows it)
    flipped = inputs.copy(); flipped[b, 0, 0, ib - 1] ^= 1
    got = _tables(ib, players, False, flipped, status, players)
    assert got[b][0] != base[b][0] and got[b][1] != base[b][1] and all(got[k] == base[k] for k in range(B) if k != b), (ib, players, "frame 0")
    # n_inputs lowered by one: the step carries it for every branch, so every branch changes (the last player's entities are skipped, everybody folds n_inputs)
    got = _tables(ib, players, False, inputs, status, players - 1)
    assert all(got[k][j] != base[k][j] for k in range(B) for j in range(T)), (ib, players, "n_inputs")
    # status NULL is every input Confirmed
    assert _tables(ib, players, False, inputs, None, players) == _tables(ib, players, False, inputs, np.zeros_like(status), players)


@pytest.mark.parametrize("ib,players", [(1, 2), (16, 3)])
def test_the_constant_index_world_reads_player_0_alone(ib, players):
    rng = np.random.default_rng([7, ib])
    inputs = rng.integers(0, 256, size=(B, T, players, ib)).astype(np.uint8)
    status = rng.integers(0, 3, size=(B, T, players)).astype(np.uint8)
    base = _tables(ib, players, True, inputs, status, players)
    a = inputs.copy(); a[1, 1, 0, 0] ^= 0x80
    got = _tables(ib, players, True, a, status, players)
    assert got[1][-1] != base[1][-1] and got[0] == base[0] and got[2] == base[2]
    st = status.copy(); st[1, 1, 0] = (st[1, 1, 0] + 1) % 3
    got = _tables(ib, players, True, inputs, st, players)
    assert got[1][-1] != base[1][-1] and got[0] == base[0] and got[2] == base[2]
    a = inputs.copy(); a[1, 1, 1:, :] ^= 0xFF                    # the other players are not read
    assert _tables(ib, players, True, a, status, players) == base
    assert _tables(ib, players, True, inputs, status, 0) != base


# ---- coverage floors over the fuzz tier's exact seeds ---------------------------------------------------------------------------------------------------------------
_RECS = {}


def _recs():
    if not _RECS:
        for s in bw.FUZZ_SEEDS: _RECS[s] = bw.fuzz_seed(s, with_lib=False)
    return [_RECS[s] for s in bw.FUZZ_SEEDS]


SAME_TABLES_CAP = 8        # steps of B >= 2 branches whose tables are all the same, counted on the oracle: the 8 of 81 that drew n_inputs = 0 (nobody reads an input)


def test_floors_of_the_branch_world_seeds():
    recs = _recs()
    assert {(r["kind"], r["layout"]) for r in recs} == set(bw.KINDS)                       # every world kind and every layout
    seen = [sum(r["stats"]["status"][k] for r in recs) for k in range(3)]
    assert all(v >= 1 for v in seen), seen                                                 # each InputStatus kind reached a (living) entity
    steps = [(r, st) for r in recs for st in r["steps"]]
    assert sum(0 < st["n_inputs"] < bw.players_of(r["kind"], r["layout"]) for r, st in steps) >= 1
    assert sum(st["n_inputs"] == 0 for r, st in steps) >= 1
    assert sum(r["with_status"] for r in recs) >= 1 and sum(not r["with_status"] for r in recs) >= 1
    same = [(r["seed"], r["kind"], st["n_inputs"]) for r, st in steps if r["B"] >= 2 and st["distinct"] < 2]
    multi = sum(r["B"] >= 2 for r, st in steps)
    print(f"{len(recs)} seeds, {len(steps)} steps, {multi} with B >= 2, of which {len(same)} have one distinct table: {same}; status kinds seen {seen}; "
          f"adoptions {sum(r['adopted'] is not None for r in recs)}, lossy {sum(r['lossy'] for r in recs)}")
    assert len(same) <= SAME_TABLES_CAP and multi >= 40, (same, multi)
    assert all(ni == 0 for _, _, ni in same), same                                         # wherever an input travels, the branches differ
    assert sum(r["lossy"] for r in recs) >= 1                                              # a lossy adoption: the documented list differs from the plain replay
    assert all(not r["lossy"] for r in recs if r["kind"] != "strategy")                    # ... and only a Strategy makes it differ
    assert sum(r["adopted"] is not None for r in recs) >= 8
    for fl in (bw.SAVE_LAST, bw.RETAIN_NEWEST, bw.RETAIN_ALL): assert sum(bool(r["flags"] & fl) for r in recs) >= 1
