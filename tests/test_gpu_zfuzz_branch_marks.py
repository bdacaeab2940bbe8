"""Branch steps and adoption on worlds with live-only state, FUZZED against the oracle's request lists (tests/test_gpu_zfuzz_branches.py is the plain-world sibling).
Per seed: the Health + non-rollback Mesh world of tests/branch_marks_common.py, or the particles world with despawn_particles written as a DEFERRING user system
plus the built-in spawn system (len grows across a unit boundary inside a branch); three consecutive branch steps with random branch counts, inputs, spawn
selections, retention flags and a random ConfirmedFrameCount lag; every Checksum(u128) of the gathered table and, after every step, the whole live state --
markers, non-rollback presence -- compared with the oracle; then a random retained branch is adopted and the session goes on for a tick.  Value tags are forced
on odd seeds; one chunk runs with kernels specialised at once (GGRS_JIT_SPECIALISE_AFTER=1, GGRS_JIT_SPECIALISE_SYNC=1)."""
import multiprocessing as mp
import os

import pytest

pytestmark = pytest.mark.gpu

SEEDS = list(range(9300, 9324))
ORACLE_CALLS = 120_000                                            # the oracle's twin of a user system is a Python callable: entity-frames per branch step


def _fuzz_rank(q, seeds):
    try:
        import numpy as np
        import bevy_ggrs_amd as bg
        import branch_marks_common as bm
        import common as cm
        from bevy_ggrs_amd import _ffi
        from bevy_ggrs_amd.fanout import RcclFanout
        from oracle.binding import FLAT, OracleWorld
        from test_despawn_rollback import state
        lib = _ffi.lib
        report = []
        for seed in seeds:
            rng = np.random.default_rng(seed)
            n = int(rng.choice([300, 1500, 6000, 40_000]))
            depth = int(rng.integers(3, 9))
            T = min(int(rng.integers(1, depth + 1)), max(1, ORACLE_CALLS // n))
            B = int(rng.choice([b for b in (1, 2, 5, 17, 40) if b == 1 or n * b * T <= ORACLE_CALLS]))
            particles = bool(rng.integers(0, 2))
            save_last = bool(rng.integers(0, 2)) or T == 1
            retain = int(rng.choice([0, _ffi.BRANCH_RETAIN_NEWEST, _ffi.BRANCH_RETAIN_ALL]))
            flags = (_ffi.BRANCH_SAVE_LAST if save_last else 0) | retain
            n_spawn = int(rng.integers(1, 80))
            steps = 3
            cap = n + n_spawn * (T + 2) * (steps + 2) + 64
            what = dict(seed=seed, n=n, depth=depth, T=T, B=B, particles=particles, flags=flags, value_tags=bool(seed % 2))

            def payload(frame):                                      # a pure function of the frame: every branch that spawns in it draws the same entities
                r = np.random.default_rng([seed, frame])
                return r.uniform(-200, 200, n_spawn).astype(np.float32), r.uniform(-200, 200, n_spawn).astype(np.float32)

            def spawn(frame, a):
                if particles and (a.inputs[0] & cm.INPUT_SPAWN): a.spawn_vx, a.spawn_vy = payload(frame)

            gw, ow = bg.World(cap, max_depth=depth + 2), OracleWorld(cap, depth + 2, FLAT)
            if seed % 2: assert lib.ggrs_dbg_set_value_tags(gw._p, 1) == 0
            ids, ttl_init = None, int(rng.integers(2, 9))
            for w in (gw, ow):
                ids = bm.build_particles_deferring(w, n, ttl_init, seed) if particles else bm.build_health(w, n)
                w.set_depth(depth + 1)
            native = RcclFanout(gw, 0, 1, RcclFanout.unique_id())
            last, conf = None, 0
            choices = [0, cm.INPUT_SPAWN] if particles else [0, 1, 2]
            for step in range(steps):
                Cf = gw.frame
                assert ow.frame == Cf
                lag = int(rng.integers(0, 3))
                conf = max(conf, Cf - lag)                            # ConfirmedFrameCount trails by 0..2 frames and never goes back
                for w in (gw, ow): w.set_confirmed(conf)
                if step == 0:
                    prefix = [bg.SaveGameState(Cf)]
                else:
                    a = bg.AdvanceFrame((int(rng.choice(choices)),)); spawn(Cf, a)
                    prefix = [bg.LoadGameState(Cf), a, bg.SaveGameState(Cf + 1)]
                F = Cf if step == 0 else Cf + 1
                pred = rng.choice(choices, size=(B, T)).astype(np.uint8)
                want = bm.oracle_walk(ow, prefix, F, pred, save_last, spawn)
                table = sel = None
                if particles:
                    table = (_ffi.BranchSpawn * T)()
                    pays = [payload(F + i) for i in range(T)]
                    for i, (vx, vy) in enumerate(pays): table[i].count, table[i].vx, table[i].vy = n_spawn, vx.ctypes.data, vy.ctypes.data
                    sel = np.where((pred & cm.INPUT_SPAWN) != 0, np.arange(1, T + 1, dtype=np.uint16)[None, :], 0).astype(np.uint16)
                rc, got = bm.library_step(native, gw, prefix, pred, flags, table, sel)
                assert rc == 0, (what, step, rc, got)
                assert len(got[0]) == len(want), (what, step, len(got[0]), len(want))
                bad = [k for k in range(len(want)) if want[k] != got[0][k]]
                assert not bad, (what, step, "first differing Checksum(u128) at", bad[0], "of", len(want))
                assert gw.frame == F == ow.frame and gw.len == ow.len, (what, step, gw.frame, F, gw.len, ow.len)
                cm.assert_states_equal(state(gw, ids), state(ow, ids), f"{what} after step {step}")
                last = (F, pred)
            F, pred = last
            adopted = None
            if retain:
                b = int(rng.integers(0, B))
                k = int(rng.integers(1, T + 1)) if retain == _ffi.BRANCH_RETAIN_ALL else T
                native.adopt(b, F + k)
                ow.handle_requests(bm.branch_requests(F, pred[b], k, save_last, T, spawn, saves=False))
                assert gw.frame == ow.frame == F + k and gw.len == ow.len, (what, "adopt", b, k, gw.frame, ow.frame, gw.len, ow.len)
                cm.assert_states_equal(state(gw, ids), state(ow, ids), f"{what} adopted branch {b} at +{k}")
                assert gw.save() == ow.save(), (what, "adopt: SaveGameState after adoption")
                for w in (gw, ow): w.set_confirmed(w.frame)
                t1 = [bg.SaveGameState(F + k), bg.AdvanceFrame((0,)), bg.SaveGameState(F + k + 1)]
                assert list(gw.handle_requests(t1)) == list(ow.handle_requests(t1)), (what, "the tick after adoption")
                cm.assert_states_equal(state(gw, ids), state(ow, ids), f"{what} the tick after adoption")
                adopted = (b, k)
            native.close()
            what["adopted"] = adopted
            report.append(what)
        q.put(("ok", report))
    except Exception as e:                                    # noqa: BLE001
        import traceback
        q.put(("error", f"{type(e).__name__}: {e}", traceback.format_exc()))


@pytest.mark.parametrize("chunk", [0, 1, 2])
def test_marker_branch_steps_and_adoption_fuzzed_against_the_oracle(chunk):
    seeds = SEEDS[chunk::3]
    env = {"GGRS_JIT_SPECIALISE_AFTER": "1", "GGRS_JIT_SPECIALISE_SYNC": "1"} if chunk == 2 else {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                                    # a spawned child inherits the parent's environment at start()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_fuzz_rank, args=(q, seeds))
    try: p.start()
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    try: r = q.get(timeout=900)
    finally:
        p.join(timeout=30)
        if p.is_alive(): p.kill()
    assert r[0] == "ok", r
    assert len(r[1]) == len(seeds)
