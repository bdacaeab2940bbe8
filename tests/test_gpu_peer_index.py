"""The peer index (ggrs_hip_register_peer_index): user systems iterate the entities that share a key with e.bucket(key) / b.count() / b.slot(i).  Everything goes
through the C ABI and is bit-exact: ggrs_hip_peer_index_read equals the numpy restatement (peer_index_common.model_index) array for array, and the Checksum(u128)
of every SaveGameState, every ring frame and the live block of the census and crowd sessions equal the CPU oracle's, whose callbacks iterate that restatement
over the oracle's own columns.  The member order -- ascending slot -- is part of the contract: the census folds it, the crowd sums f32 in it."""
import ctypes as C
import os

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
from bevy_ggrs_amd import _ffi
from oracle.binding import FLAT, OracleWorld
from peer_index_common import (CENSUS_CONFIGS, CROWD_CONFIGS, build_census, build_crowd, census_pass_out, census_session, crowd_session, model_index, run_all,
                               spawn_census, spawn_crowd, u32)

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 1025, 2048, 2049, 8300)          # across the 64-slot unit, the 256-slot workgroup, the 2048-slot sort tile and the 8192-slot layout tile
BUCKETS = (1, 2, 255, 256, 257, 65535)            # both sides of the one-pass / two-pass edge, and the maximum


def _pair(cap, depth=8):
    return bg.World(cap, max_depth=depth), OracleWorld(cap, depth, FLAT)


def _model_of_live(w, K, nb):
    n = w.len
    return model_index(w.alive_mask(n), w.present_mask(K, n), w.download_word(K, 0, 0, n), n, nb)


def _assert_index(got, want, ctx):
    assert np.array_equal(got[0], want[0]), f"{ctx}: start differs at {np.flatnonzero(got[0] != want[0])[:6]}"
    assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), f"{ctx}: slots differ at {np.flatnonzero(got[1] != want[1])[:6]}"


def _patterns(n, nb):
    i = np.arange(n, dtype=np.int64)
    return {"uniform": (i * 2654435761) % nb, "one bucket": np.full(n, nb // 2), "all out of range": np.where(i % 2 == 0, nb, 0xFFFFFFFF - i),
            "strided with holes": (i * 3) % (2 * nb)}


@pytest.mark.parametrize("nb", BUCKETS)
def test_index_read_equals_numpy(nb):
    """One world per n_buckets, grown through SIZES; at every size four key patterns (uniform; everyone in ONE bucket; everyone out of range; strided with
    holes, half of them out of range), some entities without the key component, some dead.  The whole start array and slots[:n_indexed]."""
    w = bg.World(SIZES[-1] + 40, max_depth=4)
    ids = build_census(w, nb)
    K, O, H = ids
    assert np.array_equal(w.peer_index()[0], np.zeros(nb + 1, dtype=u32)) and w.peer_index()[1].size == 0          # the empty world: nothing is launched
    cur = 0
    for n in SIZES:
        grow = n - cur
        bare = grow // 9
        w.spawn(grow - bare, {K: [np.zeros(grow - bare, dtype=u32)], O: [np.zeros(grow - bare, dtype=u32)] * 8, H: [np.full(grow - bare, 1000, dtype=u32)]})
        if bare: w.spawn(bare, {O: [np.zeros(bare, dtype=u32)] * 8, H: [np.full(bare, 1000, dtype=u32)]})
        cur = n
        if n > 64: w.despawn(n // 2); w.despawn(n - 3)
        for name, keys in _patterns(n, nb).items():
            w.upload_word(K, 0, 0, keys.astype(u32))
            got, want = w.peer_index(), _model_of_live(w, K, nb)
            _assert_index(got, want, f"n_buckets {nb}, n {n}, {name}")
            if name == "one bucket": assert got[0][-1] > 0.8 * n and got[0][nb // 2 + 1] - got[0][nb // 2] == got[0][-1]
            if name == "all out of range": assert got[0][-1] == 0
        # ... and a ring frame at this size: the frame is saved with the last pattern's keys, the live keys move on, the frame's index stays what it was
        w.handle_requests([bg.SaveGameState(w.frame)])
        want = _model_of_live(w, K, nb)
        w.upload_word(K, 0, 0, _patterns(n, nb)["uniform"].astype(u32))
        _assert_index(w.peer_index(w.frame), want, f"n_buckets {nb}, n {n}, ring frame {w.frame}")
        w.handle_requests([bg.AdvanceFrame((0,))])                            # (the next size saves the next frame)
    info = w.kernel_info()
    assert info["peer_index"].startswith(f"{nb} buckets"), info


def test_index_of_every_ring_frame_and_of_the_live_world():
    n, nb = 600, 40
    g = bg.World(n + 16, max_depth=8)
    run_all(census_session(g, n, nb, 4, 9, n_bare=20))
    K = 0
    _assert_index(g.peer_index(bg.LIVE), _model_of_live(g, K, nb), "live")
    frames = [f for f in range(g.frame + 1) if g.has_snapshot(f)]
    assert len(frames) >= 4
    seen = set()
    for f in reversed(frames):                                               # newest first: a Load pops the newer snapshots
        got = g.peer_index(f)
        g.load(f)
        _assert_index(got, _model_of_live(g, K, nb), f"ring frame {f}")
        seen.add(got[1].tobytes())
    assert len(seen) > 1                                                     # the frames' indexes differ: rekey moves everyone every frame
    with pytest.raises(bg.GgrsHipError) as e: g.peer_index(g.frame + 50)
    assert e.value.code == bg.GGRS_E_NO_SNAPSHOT


def test_index_read_is_refused_while_lists_are_uncollected():
    n, nb = 100, 7
    g = bg.World(n + 16, max_depth=4)
    ids = build_census(g, nb); spawn_census(g, ids, n, nb)
    g.set_depth(4); g.set_synctest_check_distance(-1)
    g.handle_requests([bg.SaveGameState(0)])
    g.enqueue_requests([bg.AdvanceFrame((0,)), bg.SaveGameState(1)])
    with pytest.raises(bg.GgrsHipError) as e: g.peer_index()
    assert e.value.code == bg.GGRS_E_INVALID and "uncollected" in str(e.value)
    g.collect_checksums()
    _assert_index(g.peer_index(), _model_of_live(g, ids[0], nb), "after collect")


def test_registering_after_seal_is_refused():
    w = bg.World(64, max_depth=4)
    K = w.register_component("Key", 4, 1); O = w.register_component("Out", 4, 1)
    w.checksum_component(O, [0])
    w.spawn(4, {K: [np.zeros(4, dtype=u32)], O: [np.zeros(4, dtype=u32)]})
    w.handle_requests([bg.SaveGameState(0)])                                    # seals the world
    with pytest.raises(bg.GgrsHipError) as e: w.register_peer_index(K, 0, 8)
    assert e.value.code == bg.GGRS_E_INVALID and "register_peer_index after the world was sealed" in str(e.value)
    assert w._lib.ggrs_hip_peer_index_read(w._p, bg.LIVE, None, None, None) == bg.GGRS_E_INVALID and b"no peer index" in w._lib.ggrs_hip_last_error(w._p)


def _compare(a, b, ctx):
    assert len(a[0]) == len(b[0]) > 0, (len(a[0]), len(b[0]))
    for (fa, ca), (fb, cb) in zip(a[0], b[0]):
        assert fa == fb and ca == cb, f"{ctx}: frame {fa}: gpu {ca:#x} oracle {cb:#x}"
    cm.assert_states_equal(a[1], b[1], ctx)


def _ring_and_live(g, o, ids, ctx):
    cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ids), f"{ctx}: live")
    frames = [f for f in range(g.frame + 1) if g.has_snapshot(f)]
    assert frames and frames == [f for f in range(o.frame + 1) if o.has_snapshot(f)]
    for f in reversed(frames):
        g.load(f); o.load(f)
        cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ids), f"{ctx}: ring frame {f}")


def _is_index_world(w, launches_per_build):
    """launches_per_build: 4 (n_buckets <= 255) or 7 in the large form; a world of at most 2048 slots takes the one-launch sort: 2 (k_ix_small, k_ix_bounds)"""
    if w.len <= 2048: launches_per_build = 2
    info = w.kernel_info()
    assert info["request_group_kernel"].startswith("ggrs_jit_tick") and info["group_caps"].endswith("/ 1 steps"), info
    import re
    m = re.search(r"\((\d+) builds, (\d+) launches so far\)", info["peer_index"])
    assert m and int(m.group(1)) > 0 and int(m.group(2)) == launches_per_build * int(m.group(1)), info["peer_index"]


@pytest.mark.parametrize("name", list(CENSUS_CONFIGS))
def test_census_synctest_against_the_oracle(name):
    """Every Save's checksum, then the live block and every ring frame downloaded and compared.  "spawns": host-decided children land in existing buckets from
    the next frame on.  "edits": between lists a key is uploaded out of range, the key component removed and inserted, a member despawned."""
    n, nb, cd, ticks, kw = CENSUS_CONFIGS[name]
    g, o = _pair(n + 128)
    a = run_all(census_session(g, n, nb, cd, ticks, check=lambda w: _is_index_world(w, 4 if nb <= 255 else 7), **kw))
    b = run_all(census_session(o, n, nb, cd, ticks, **kw))
    assert len(a) == len(b) > ticks - 1
    for (fa, ca), (fb, cb) in zip(a, b): assert fa == fb and ca == cb, f"census {name}: frame {fa}: gpu {ca:#x} oracle {cb:#x}"
    _ring_and_live(g, o, (0, 1, 2), f"census {name}")
    if kw.get("with_spawn"): assert g.len > n
    out0 = g.download_word(1, 0, 0, n)
    assert (out0[g.alive_mask(n)] >= 2).any()                                 # somebody saw a bucket with company


@pytest.mark.parametrize("name", list(CROWD_CONFIGS))
def test_crowd_synctest_against_the_oracle(name):
    n, gw, gh, cd, ticks, seed, span = CROWD_CONFIGS[name]
    g, o = _pair(n + 32)
    a = run_all(crowd_session(g, n, gw, gh, cd, ticks, seed=seed, n_bare=n // 50, span=span))
    b = run_all(crowd_session(o, n, gw, gh, cd, ticks, seed=seed, n_bare=n // 50, span=span))
    assert len(a) == len(b) > 0
    for (fa, ca), (fb, cb) in zip(a, b): assert fa == fb and ca == cb, f"crowd {name}: frame {fa}: gpu {ca:#x} oracle {cb:#x}"
    _ring_and_live(g, o, (0, 1, 2, 3), f"crowd {name}")
    _is_index_world(g, 7)
    key = g.download_word(2, 0, 0, n)
    assert (key == gw * gh).any() and (key < gw * gh).sum() > n // 2            # some left the field (in no bucket), most are inside


def _p2p_lists(ticks, seed=9):
    rng = np.random.default_rng(seed)
    out, F = [], 0
    for _ in range(ticks):
        k = int(min(rng.integers(0, 5), F))
        reqs = [bg.LoadGameState(F - k)]
        for i in range(k + 1):
            reqs += [bg.AdvanceFrame((((F - k + i) * 7) & 3,)), bg.SaveGameState(F - k + i + 1)]
        out.append((F, k, reqs))
        F += 1
    return out


def test_crowd_p2p_shaped_lists_two_in_flight():
    n, gw, gh = 700, 16, 16
    g, o = _pair(n + 16, depth=8)
    lists = _p2p_lists(12)
    got, want = [], []
    ids = build_crowd(g, gw, gh); spawn_crowd(g, ids, n, gw, gh, 5, n_bare=20)
    g.set_depth(8); g.set_synctest_check_distance(-1)
    got += g.handle_requests([bg.SaveGameState(0)])
    inflight = 0
    for F, k, reqs in lists:
        if F - 8 >= 0: g.set_confirmed(F - 8)
        g.enqueue_requests(reqs); inflight += 1
        if inflight == 2: got += g.collect_checksums(); inflight -= 1
    while inflight: got += g.collect_checksums(); inflight -= 1
    ido = build_crowd(o, gw, gh); spawn_crowd(o, ido, n, gw, gh, 5, n_bare=20)
    o.set_depth(8)
    want += o.handle_requests([bg.SaveGameState(0)])
    for F, k, reqs in lists:
        if F - 8 >= 0: o.set_confirmed(F - 8)
        for r in reqs: want += o.handle_requests([r])
    assert len(got) == len(want) == 1 + sum(k + 1 for _, k, _ in lists) and len({k for _, k, _ in lists}) >= 4
    assert got == want
    cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), "p2p-shaped lists")


def test_crowd_with_specialised_copies_forced_at_first_sight(monkeypatch):
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    n, gw, gh = 400, 16, 16
    g, o = _pair(n + 16)
    assert g._lib.ggrs_dbg_set_spec_shapes(g._p, 3) == 0
    a = run_all(crowd_session(g, n, gw, gh, 2, 8, seed=6))
    spec = g.kernel_info()
    b = run_all(crowd_session(o, n, gw, gh, 2, 8, seed=6))
    assert spec["specialised_kernel"].startswith("ready"), spec["specialised_kernel"]
    assert a == b
    cm.assert_states_equal(cm.snapshot_state(g, (0, 1, 2, 3)), cm.snapshot_state(o, (0, 1, 2, 3)), "specialised copies")


def test_a_group_that_opens_with_a_load_builds_the_index_from_the_ring_slot():
    """Expected values from the numpy restatement over the INITIAL state, no oracle: after one frame rekey has moved every key, so an index built from the live
    block would differ; [Load(0), Advance] must write what the first Advance wrote."""
    n, nb = 200, 9
    w = bg.World(n + 8, max_depth=4)
    ids = build_census(w, nb); spawn_census(w, ids, n, nb, n_bare=6)
    K, O, H = ids
    want = census_pass_out(w.alive_mask(n), w.present_mask(K, n), w.download_word(K, 0, 0, n), n, nb)
    out = lambda: np.stack([w.download_word(O, k, 0, n) for k in range(8)], axis=1).astype(np.uint64)
    w.handle_requests([bg.SaveGameState(0), bg.AdvanceFrame((0,))])
    first = out()
    assert np.array_equal(first, want)
    w.handle_requests([bg.SaveGameState(1), bg.AdvanceFrame((0,))])
    assert not np.array_equal(out(), first)                                 # frame 2 saw other buckets
    w.handle_requests([bg.LoadGameState(0), bg.AdvanceFrame((0,))])           # the rollback re-simulates frame 1 from ITS snapshot
    assert np.array_equal(out(), want)


def _fanout_rank(q, lib_path):
    try:
        os.environ["GGRS_RCCL_LIB"] = lib_path
        from bevy_ggrs_amd.fanout import RcclFanout
        n, nb = 300, 24
        g, o = _pair(n + 16)
        ids = build_census(g, nb); spawn_census(g, ids, n, nb)
        ido = build_census(o, nb); spawn_census(o, ido, n, nb)
        for w in (g, o): w.set_depth(6)
        native = RcclFanout(g, 0, 1, RcclFanout.unique_id())
        pre, keep, _ = g.build_requests([bg.SaveGameState(0)])
        inputs = np.zeros((2, 2, 1), dtype=np.uint8)
        bs = _ffi.BranchStep()
        bs.prefix, bs.n_prefix, bs.n_branches, bs.n_frames, bs.n_inputs, bs.flags = pre, 1, 2, 2, 1, _ffi.BRANCH_SAVE_LAST
        bs.inputs = inputs.ctypes.data
        rc = _ffi.lib.ggrs_hip_fanout_step_branches(native._p, C.byref(bs), None)
        msg = (_ffi.lib.ggrs_hip_fanout_last_error(native._p) or b"").decode()
        reqs = [bg.SaveGameState(0)]
        for b in range(2):
            reqs += [bg.LoadGameState(0), bg.AdvanceFrame((b + 1,)), bg.SaveGameState(1), bg.AdvanceFrame((b + 1,)), bg.SaveGameState(2)]
        ns = native.step(reqs)
        table = native.collect()
        got = [int(p[0]) | (int(p[1]) << 64) for p in table.reshape(-1, 2)]
        want = []
        for r in reqs: want += o.handle_requests([r])
        same = True
        try: cm.assert_states_equal(cm.snapshot_state(g, ids), cm.snapshot_state(o, ido), "fan-out")
        except AssertionError: same = False
        native.close()
        q.put(("ok", rc, msg, ns, got, want, same))
    except Exception as e:                                    # noqa: BLE001
        import traceback
        q.put(("error", f"{type(e).__name__}: {e}", traceback.format_exc()))


def test_branch_steps_are_refused_and_the_request_list_form_works():
    import multiprocessing as mp
    from test_gpu_zfanout import _double_lib                                                   # (a name only: no test is imported)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_fanout_rank, args=(q, _double_lib())); p.start()
    try: r = q.get(timeout=300)
    finally:
        p.join(timeout=60)
        if p.is_alive(): p.kill()
    assert r[0] == "ok", r
    _, rc, msg, ns, got, want, same = r
    assert rc == bg.GGRS_E_INVALID and "peer bindings" in msg and "ggrs_hip_fanout_step" in msg, (rc, msg)
    assert ns == 5 and got == want and same, (ns, got, want, same)
