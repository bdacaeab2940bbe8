"""ggrs_hip_fanout_step_branches / ggrs_hip_fanout_adopt FUZZED over the worlds test_gpu_zfuzz_branches.py does not reach (tests/branch_worlds_common.py): inputs of
1..16 bytes for 1..5 players read through a handle or a constant index, InputStatus bytes (or NULL), n_inputs below the players of the session (0 included), a
component under a lossy Strategy, narrow words, a user-written hasher, box_game.  Per seed: three consecutive branch steps behind a prefix, every Checksum(u128) of
the gathered table, the live state, the frame and len compared with the oracle walking the same branches as request lists; then, where the step retained, a random
branch is adopted at a random retained frame and the whole live state, SaveGameState and the tick after are compared with the list include/ggrs_hip.h documents
adoption to equal (branch_worlds_common.adoption_requests).  Value tags and the lazy live block are forced on odd seeds.

Seed i runs kind i % 12, so a chunk's process builds each of its four kernel texts once.  tests/test_branch_worlds.py runs the same generator with the oracle alone
and holds its coverage floors."""
import pytest

pytestmark = pytest.mark.gpu


def _fuzz_rank(q, seeds):
    try:
        import branch_worlds_common as bw
        report = []
        for seed in seeds:
            rec = bw.fuzz_seed(seed, with_lib=True)
            report.append({k: rec[k] for k in ("seed", "kind", "layout", "n", "T", "B", "flags", "adopted", "lossy")})
        q.put(("ok", report))
    except Exception as e:                                    # noqa: BLE001
        import traceback
        q.put(("error", f"{type(e).__name__}: {e}", traceback.format_exc()))


@pytest.mark.parametrize("chunk", [0, 1, 2])
def test_branch_steps_over_wide_inputs_status_and_strategy_fuzzed_against_the_oracle(chunk):
    import branch_worlds_common as bw
    seeds = bw.FUZZ_SEEDS[chunk::3]
    r = bw.run_in_process(_fuzz_rank, seeds, timeout=900)
    assert r[0] == "ok", r
    assert len(r[1]) == len(seeds)
