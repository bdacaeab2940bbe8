"""ggrs_hip_fanout_step_branches over what its other tests leave out (they all pass n_inputs = 1, one byte per input, status = NULL): named cases, each the
checksum table, the live state, the frame and len after the step, bit-exact against the oracle's list form (tests/branch_worlds_common.py).

  * input layouts (bytes, players) of 1 x 2, 2 x 5, 4 x 3, 8 x 1, 16 x 3 -- rows of 4, 15, 15, 9 and 51 bytes behind the n_inputs bytes of a member record, unaligned --
    x n_inputs in {0 (inputs = NULL), 1, players} x status in {NULL, random}: B = 5, T = 3, n = 257 (1, 65, 257 and 2100 for 2 x 5 and 16 x 3: a lone entity, past one
    wave, past one four-unit tile, past the eighth tile);
  * an InputStatus byte outside the enum in the last branch's last frame: GGRS_E_INVALID before the prefix runs;
  * a world with a component under a lossy Strategy: retention-free steps, both retaining flags refused without GGRS_BRANCH_SAVE_LAST, adoption of a block that
    holds Strategy::Stored -- value tags off and forced on;
  * the narrow-word world, the user-written hasher and box_game (2 and 4 players): B = 8, T = 4, with and without GGRS_BRANCH_RETAIN_ALL + adoption.
One process per group of cases (its own HIP context and RCCL communicator)."""
import pytest

pytestmark = pytest.mark.gpu

ALL_N = [1, 65, 257, 2100]


def _reply(q, fn, *args):
    try: q.put(("ok", fn(*args)))
    except Exception as e:                                    # noqa: BLE001
        import traceback
        q.put(("error", f"{type(e).__name__}: {e}", traceback.format_exc()))


def _layout_cases(kind, layout, ns):
    import re
    import numpy as np
    import bevy_ggrs_amd as bg
    import branch_worlds_common as bw
    B, T = 5, 3
    done = []
    for n in ns:
        s = bw.Session(kind, layout, n, 4, True)
        rng = np.random.default_rng([layout[0], layout[1], n])
        case = 0
        for n_inputs in sorted({0, 1, s.players}):
            for with_status in (False, True):
                Cf = s.ow.frame
                prefix = [bg.LoadGameState(Cf), s.rand_advance(rng, s.players), bg.SaveGameState(Cf + 1)] if case else [s.rand_advance(rng, s.players), bg.SaveGameState(Cf + 1)]
                inputs = s.rand_inputs(rng, B, T)
                status = rng.integers(0, 3, size=(B, T, s.players)).astype(np.uint8) if with_status else None
                per = s.step(prefix, inputs, status, n_inputs, bw.SAVE_LAST if case % 3 else 0, ctx=f"n_inputs={n_inputs} status={with_status}")
                assert len({tuple(p) for p in per}) == (B if n_inputs else 1), (s.what, n_inputs, "branches whose player 0 differs must differ in their tables")
                case += 1; done.append((n, n_inputs, with_status))
        # an InputStatus byte outside the enum, in the last branch's last frame: refused before the prefix runs (refused() checks that frame and len stand)
        Cf = s.ow.frame
        status = rng.integers(0, 3, size=(B, T, s.players)).astype(np.uint8); status[B - 1, T - 1, s.players - 1] = 3
        rc, msg = s.refused([bg.LoadGameState(Cf), s.rand_advance(rng, s.players), bg.SaveGameState(Cf + 1)], s.rand_inputs(rng, B, T), status, s.players, bw.SAVE_LAST)
        assert rc == bg.GGRS_E_INVALID and re.search(r"InputStatus 3 is none of", msg), (rc, msg)
        assert s.gw.frame == Cf == s.ow.frame
        s.same_state("after the refused step")
        s.close()
    return done


@pytest.mark.parametrize("ib,players", [(1, 2), (2, 5), (4, 3), (8, 1), (16, 3)])
def test_input_layouts_n_inputs_and_status_reach_every_branch_frame(ib, players):
    import branch_worlds_common as bw
    ns = ALL_N if (ib, players) in ((2, 5), (16, 3)) else [257]
    r = bw.run_in_process(_reply, _layout_cases, "inputs", (ib, players), ns, timeout=600)
    assert r[0] == "ok", r
    assert len(r[1]) == len(ns) * (4 if players == 1 else 6)


@pytest.mark.parametrize("ib,players", [(1, 2), (16, 3)])
def test_a_constant_input_index_in_a_branch_step(ib, players):
    import branch_worlds_common as bw
    r = bw.run_in_process(_reply, _layout_cases, "const", (ib, players), [257], timeout=600)
    assert r[0] == "ok", r
    assert len(r[1]) == 6


def _strategy_cases(vtags):
    import re
    import numpy as np
    import bevy_ggrs_amd as bg
    import branch_worlds_common as bw
    B, T, n = 5, 3, 257
    s = bw.Session("strategy", (1, 16), n, 5, True, vtags=vtags)
    A = s.ids[0]
    rng = np.random.default_rng(17 + vtags)

    def step(flags, first=False):
        Cf = s.ow.frame
        prefix = [s.rand_advance(rng, 1), bg.SaveGameState(Cf + 1)] if first else [bg.LoadGameState(Cf), s.rand_advance(rng, 1), bg.SaveGameState(Cf + 1)]
        return prefix, s.rand_inputs(rng, B, T), rng.integers(0, 3, size=(B, T, s.players)).astype(np.uint8)

    for k, flags in enumerate((0, bw.SAVE_LAST)):                                            # retention-free, without and with the last Save
        prefix, inputs, status = step(flags, first=not k)
        per = s.step(prefix, inputs, status, 1, flags, ctx=f"flags={flags}")
        assert len({tuple(p) for p in per}) > 1
    for flags in (bw.RETAIN_NEWEST, bw.RETAIN_ALL):                                          # a retained live-form block could not become a ring slot: refused
        prefix, inputs, status = step(flags)
        rc, msg = s.refused(prefix, inputs, status, 1, flags)
        assert rc == bg.GGRS_E_INVALID and re.search(r"Strategy .*GGRS_BRANCH_SAVE_LAST", msg), (rc, msg)
    out = []
    for flags, b, k in ((bw.RETAIN_NEWEST | bw.SAVE_LAST, 3, T), (bw.RETAIN_ALL | bw.SAVE_LAST, 1, 2), (bw.RETAIN_ALL | bw.SAVE_LAST, 4, T)):
        prefix, inputs, status = step(flags)
        s.step(prefix, inputs, status, 1, flags, ctx=f"flags={flags}")
        diff = s.adopt(b, k, s.rand_advance(rng, 1))
        # the oracle alone: the list adoption is documented to equal differs from the plain replay in the lossy word, and in no other (x is exact in f16, z was
        # rounded by the LoadGameState the branch started with)
        assert diff == [f"c{A}w1"], diff
        out.append((flags, b, k))
    s.close()
    return out


@pytest.mark.parametrize("vtags", [0, 1])
def test_strategy_world_branch_steps_refusals_and_adoption_of_a_stored_block(vtags):
    """The oracle side of an adoption is the list include/ggrs_hip.h documents for ggrs_hip_fanout_adopt -- "a snapshot of `frame` in the ring, the live world loaded
    from it (what LoadGameState leaves behind)" --: [LoadGameState(F), AdvanceFrame x k, SaveGameState(F + k), LoadGameState(F + k)] with the adopted branch's inputs
    (branch_worlds_common.adoption_requests).  For Accel.y it differs from the plain replay [LoadGameState(F), AdvanceFrame x k], which the test asserts on the oracle."""
    import branch_worlds_common as bw
    r = bw.run_in_process(_reply, _strategy_cases, vtags, timeout=600)
    assert r[0] == "ok", r
    assert len(r[1]) == 3


def _strategy_live_after_a_step():
    import numpy as np
    import bevy_ggrs_amd as bg
    import branch_worlds_common as bw
    s = bw.Session("strategy", (1, 16), 65, 3, True)
    rng = np.random.default_rng(3)
    A = s.ids[0]
    for w in s.worlds(): w.handle_requests([s.rand_advance(np.random.default_rng(4), 1)])
    before = bw.cm.snapshot_state(s.ow, s.ids)
    s.step([bg.SaveGameState(1)], s.rand_inputs(rng, 2, 1), None, 1, bw.SAVE_LAST, ctx="the prefix does not load")       # (step compares the live state)
    after = bw.cm.snapshot_state(s.ow, s.ids)
    assert not np.array_equal(before[f"c{A}w1"], after[f"c{A}w1"])                # on the oracle alone: the closing LoadGameState(F) rounds the lossy word
    s.close()
    return True


def test_a_branch_step_leaves_a_strategy_world_as_the_closing_load_of_the_list_form_does():
    """Regression: a prefix that ends with SaveGameState(F) without a LoadGameState before it leaves the live world in the component's own form; the list form of the
    step ends with LoadGameState(F), which leaves load(store(x)).  The branch step used to leave the former (Accel.y unrounded); it now ends with that LoadWorld."""
    import branch_worlds_common as bw
    r = bw.run_in_process(_reply, _strategy_live_after_a_step, timeout=600)
    assert r == ("ok", True), r


def _retain_cases(kind, layout):
    import numpy as np
    import bevy_ggrs_amd as bg
    import branch_worlds_common as bw
    B, T, n = 8, 4, 300
    s = bw.Session(kind, layout, n, 6, True)
    rng = np.random.default_rng([B, T, layout[1]])
    out = []
    for case, (flags, adopt) in enumerate(((0, None), (bw.SAVE_LAST, None), (bw.RETAIN_ALL, (6, T)), (bw.RETAIN_ALL | bw.SAVE_LAST, (2, 2)))):
        Cf = s.ow.frame
        prefix = [bg.LoadGameState(Cf), s.rand_advance(rng, s.players), bg.SaveGameState(Cf + 1)] if case else [s.rand_advance(rng, s.players), bg.SaveGameState(Cf + 1)]
        inputs = s.rand_inputs(rng, B, T)
        status = rng.integers(0, 3, size=(B, T, s.players)).astype(np.uint8) if case % 2 else None
        per = s.step(prefix, inputs, status, s.players, flags, ctx=f"flags={flags}")
        assert len({tuple(p) for p in per}) > 1, (s.what, "the branches do not diverge")
        if adopt:
            assert s.adopt(adopt[0], adopt[1], s.rand_advance(rng, s.players)) == []         # no Strategy: the documented list is the plain replay
        out.append((flags, adopt))
    s.close()
    return out


@pytest.mark.parametrize("kind,players", [("narrow", 16), ("hasher", 16), ("box", 2), ("box", 4)])
def test_schema_worlds_and_box_game_in_branch_steps_with_and_without_retention(kind, players):
    import branch_worlds_common as bw
    r = bw.run_in_process(_reply, _retain_cases, kind, (1, players), timeout=600)
    assert r[0] == "ok", r
    assert len(r[1]) == 4
