"""The census world under the request fuzzer on the CPU (tests/fuzz_peer_index.py): the seeds the GPU tier runs (test_gpu_zfuzz_peer_index.py), here on the
oracle's two storage modes -- FLAT against REFSHAPED behind enqueue / collect, the stream the HIP backend gets -- and held to coverage floors counted on the oracle
alone, so that the device tier cannot go hollow.

The committed seeds: fuzz_peer_index.SEEDS = 0 .. 23 over SIZES (1, 2, 63, 64, 65, 257, 1025) and TILE = seed 3 at n = 8262, 5 lists.  Summed over them the
oracle sees at least: 150 AdvanceFrames whose index has a bucket with two members or more, 150 with a visible key out of range, 12 host edits that take a member
out of the index, and 12 Loads followed by an AdvanceFrame whose index differs from the live world's."""
import pytest

import fuzz_peer_index as fp
import fuzz_user_worlds as fu

FLOORS = {"multi": 150, "out_of_range": 150, "lost": 12, "load_differs": 12}


@pytest.fixture(scope="module")
def sessions():
    out = {}
    for seed in fp.SEEDS: out[seed] = fp.cpu_pair(seed)
    seed, n, n_lists = fp.TILE
    out["tile"] = fp.cpu_pair(seed, n=n, n_lists=n_lists)
    return out


def test_the_committed_seeds_meet_every_coverage_floor(sessions):
    total = {k: sum(getattr(st, k) for _, _, st in sessions.values()) for k in FLOORS}
    adv = sum(st.advances for _, _, st in sessions.values())
    print(total, adv)
    for k, floor in FLOORS.items(): assert total[k] >= floor, (k, total)
    sizes = {sc.n for _, sc, _ in sessions.values()}
    assert sizes >= {1, 63, 64, 65, 257, 1025, 8262} and {sc.nb for _, sc, _ in sessions.values()} == {3, 40, 300}


def test_the_sessions_hold_the_shapes_the_scripted_ones_never_send(sessions):
    mid = twice = branch = 0
    for log, _, _ in sessions.values():
        a, b, c = fu.shapes(log); mid += a; twice += b; branch += c
    assert mid >= 20 and twice >= 10 and branch >= 5, (mid, twice, branch)
    log, sc, st = sessions["tile"]
    assert sc.n == 8262 and 0 < fu.advances(log) <= 40, (log[0], fu.advances(log))
