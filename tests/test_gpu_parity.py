"""HIP path vs CPU oracle through the C ABI, bit-exact (integer checksums, masks, counters, and
f32 columns compared as raw bits: the checksum hashes f32 bits, so 1 ULP is already a failure)."""
import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
from oracle.binding import FLAT, OracleWorld

pytestmark = pytest.mark.gpu


def _pair(capacity, depth=16, flags=0):
    return bg.World(capacity, max_depth=depth, flags=flags), OracleWorld(capacity, depth, FLAT)


def _run(world, n, cd, ticks, ttl_mode="despawn", with_spawn=True, ttl_init=40, spawn_every=3, rate=100):
    vel, ttl = cm.synthetic_particles(n, ttl=ttl_mode)
    ids = cm.build_particles(world, with_spawn=with_spawn, ttl_init=ttl_init)
    cm.spawn_particles(world, ids, n, vel, ttl)
    drv = cm.SyncTestDriver(world, cd)
    fn = cm.frame_spawn_fn(rate)
    for t in range(ticks):
        drv.tick((cm.INPUT_SPAWN if (with_spawn and t % spawn_every == 1) else 0,), spawn_fn=fn)
    return drv.all_checksums, cm.snapshot_state(world, ids)


@pytest.mark.parametrize("n,cd,ticks", [(1, 2, 12), (63, 1, 10), (1000, 2, 20), (1025, 7, 24), (10_000, 8, 30), (100_000, 8, 14)])
@pytest.mark.parametrize("flags", [0, bg.GGRS_WORLD_NO_GROUPS, bg.GGRS_WORLD_UNFUSED])
def test_particles_synctest_checksums_and_state(n, cd, ticks, flags):
    cap = n + 100 * ticks + 64
    g, o = _pair(cap, 16, flags)
    a = _run(g, n, cd, ticks)
    b = _run(o, n, cd, ticks)
    assert len(a[0]) == len(b[0]) > 0
    for (fa, ca), (fb, cb) in zip(a[0], b[0]):
        assert fa == fb and ca == cb, f"frame {fa}: gpu {ca:#x} oracle {cb:#x}"
    cm.assert_states_equal(a[1], b[1], f"n={n} cd={cd}")


def test_600_frames_bit_exact_f32():
    """every f32 bit-equal over >= 600 frames (no FMA contraction,
    -0.0 + 0.0 handling, dt alternation)."""
    n = 5000
    vel, ttl = cm.synthetic_particles(n, ttl="throughput")
    vel[::7, 0] = -0.0                              # x += +0.0 must turn -0.0 into +0.0
    vel[::11, 1] = np.float32(1e-38)                # subnormal-adjacent inputs
    worlds = _pair(n)
    cs = []
    for w in worlds:
        ids = cm.build_particles(w)
        cm.spawn_particles(w, ids, n, vel, ttl)
        out = []
        for f in range(600):
            w.advance()
            if f % 50 == 49: out.append(w.save())
        cs.append((out, cm.snapshot_state(w, ids)))
    assert cs[0][0] == cs[1][0]
    cm.assert_states_equal(cs[0][1], cs[1][1], "600 frames")


def test_empty_world_and_ragged_sizes():
    for n in (0, 1, 64, 65, 1023, 1024, 1025, 4097):
        g, o = _pair(max(n, 1) + 10)
        res = []
        for w in (g, o):
            ids = cm.build_particles(w)
            if n:
                vel, ttl = cm.synthetic_particles(n, ttl="despawn")
                cm.spawn_particles(w, ids, n, vel, ttl)
            c0 = w.save(); w.advance(); c1 = w.save(); w.load(0); c2 = w.save()
            res.append((c0, c1, c2, cm.snapshot_state(w, ids)))
        assert res[0][:3] == res[1][:3], n
        assert res[0][0] == res[0][2], "load(0) then save must reproduce the frame-0 checksum"
        cm.assert_states_equal(res[0][3], res[1][3], f"n={n}")


def test_disjoint_components_and_presence_masks():
    """benches/bench.rs:68-95 foo_bar_baz: entities with disjoint component sets; plus
    insert/remove of a component across a rollback (component_snapshot.rs:106-115)."""
    res = []
    for w in _pair(4000):
        foo = w.register_component("Foo", 4, 1); bar = w.register_component("Bar", 4, 1); baz = w.register_component("Baz", 4, 1)
        for c in (foo, bar, baz): w.checksum_component(c, [0])
        w.add_system(bg.SYS_ADD_U32, comp=(foo,), word=(0,), iparam=(1,))
        w.add_system(bg.SYS_ADD_U32, comp=(bar,), word=(0,), iparam=(-1 & 0xFFFFFFFF,))
        w.add_system(bg.SYS_ADD_U32, comp=(baz,), word=(0,), iparam=(1,))
        v = np.arange(1000, dtype=np.uint32)
        w.spawn(1000, {foo: [v]}); w.spawn(1000, {bar: [v]}); w.spawn(1000, {baz: [v]})
        out = [w.save()]                              # frame 0
        w.advance(); out.append(w.save())             # frame 1
        w.remove_component(foo, 5); w.insert_component(bar, 5, np.array([77], np.uint32)); w.despawn(1500)
        w.advance(); out.append(w.save())             # frame 2
        w.load(1); out.append(w.save())               # back: foo present on 5 again, bar absent, 1500 alive
        w.advance(); out.append(w.save())
        res.append((out, cm.snapshot_state(w, (foo, bar, baz))))
    assert res[0][0] == res[1][0]
    assert res[0][0][1] == res[0][0][3]
    cm.assert_states_equal(res[0][1], res[1][1], "disjoint")


def test_generic_checksum_u64_words_and_mixed_specs():
    """checksum spec over a u64 column (Ttl) and a non-prefix word subset -> generic k_checksum."""
    res = []
    n = 3000
    vel, ttl = cm.synthetic_particles(n, ttl="despawn")
    for w in _pair(n):
        T, V, L = cm.build_particles(w, checksum=False)
        w2 = w
        # registration is still open (no spawn yet)
        w2.checksum_component(L, [0])
        w2.checksum_component(T, [2, 0, 9, 6])
        cm.spawn_particles(w, (T, V, L), n, vel, ttl)
        out = []
        for _ in range(5):
            w.advance(); out.append(w.save())
        res.append(out)
    assert res[0] == res[1]


def test_errors_match_reference_panics():
    g = bg.World(100, max_depth=4)
    g.register_component("X", 4, 1)
    g.save()
    with pytest.raises(bg.GgrsHipError) as e:
        g.load(99)                                   # mod.rs:213 panic -> GGRS_E_NO_SNAPSHOT
    assert e.value.code == bg.GGRS_E_NO_SNAPSHOT and "Could not rollback to 99" in str(e.value)
    assert g.snapshot_count() == 0                   # the reference's loop popped everything first
    with pytest.raises(bg.GgrsHipError) as e:
        g.spawn(101, {0: None})
    assert e.value.code == bg.GGRS_E_CAPACITY
    with pytest.raises(bg.GgrsHipError):
        g.register_component("late", 4, 1)           # registration after seal


@pytest.mark.parametrize("n,ticks", [(300_000, 12), (600_000, 12), (1_000_000, 12), (4_000_000, 11)])
@pytest.mark.parametrize("ttl_mode", ["despawn"])
def test_headline_depth8_matches_oracle(n, ticks, ttl_mode):
    """BASELINE config 3 at its own size and the sizes either side of the generated kernel's policy thresholds (host_groups.hpp:
    cached vs non-temporal snapshot stores at 416 k slots, the first Save through the L2 up to 80 MB of rows, the on-chip group fold
    from 12288 workgroups = 3 M slots), DEFAULT dispatch, SyncTest check distance 8 with max_prediction 9: every Save's
    Checksum(u128) == the oracle's (component_checksum.rs:67-108, tests/synctest.rs:84-125) and the final live state is byte-equal."""
    from oracle.binding import lib as olib
    import os
    olib.gor_set_num_threads(max(1, min(32, len(os.sched_getaffinity(0)))))
    try:
        vel, ttl = cm.synthetic_particles(n, ttl=ttl_mode)
        res = []
        for w in (bg.World(n, max_depth=9), OracleWorld(n, 9, FLAT)):
            ids = cm.build_particles(w)
            cm.spawn_particles(w, ids, n, vel, ttl)
            drv = cm.SyncTestDriver(w, 8, max_prediction=9)
            for _ in range(ticks):
                drv.tick((0,))
            res.append((drv.all_checksums, cm.snapshot_state(w, ids)))
            w.close()
    finally:
        olib.gor_set_num_threads(max(1, min(8, len(os.sched_getaffinity(0)))))
    a, b = res
    assert len(a[0]) == len(b[0]) >= 8 * (ticks - 9)
    for (fa, ca), (fb, cb) in zip(a[0], b[0]):
        assert fa == fb and ca == cb, f"n={n} frame {fa}: gpu {ca:#x} oracle {cb:#x}"
    cm.assert_states_equal(a[1], b[1], f"headline n={n}")


def test_full_size_properties_1m():
    """BASELINE config 3 (1M x 3 components, depth 8): size-independent properties instead of
    the (slow) oracle: resimulation reproduces every first-recorded checksum (the SyncTest
    driver would raise MismatchedChecksum), load(f)+save == saved checksum, and fused ==
    unfused kernels."""
    n = 1_000_000
    vel, ttl = cm.synthetic_particles(n, ttl="despawn")
    outs = []
    for flags in (0, bg.GGRS_WORLD_NT_COPY, bg.GGRS_WORLD_NO_GROUPS, bg.GGRS_WORLD_UNFUSED):
        w = bg.World(n, max_depth=9, flags=flags)
        ids = cm.build_particles(w)
        cm.spawn_particles(w, ids, n, vel, ttl)
        drv = cm.SyncTestDriver(w, 8, max_prediction=9)
        for _ in range(12):
            drv.tick((0,))
        outs.append(drv.all_checksums)
        first = {}
        for f, c in drv.all_checksums:
            assert first.setdefault(f, c) == c
        f_old = w.frame - 3
        want = first[f_old]
        w.load(f_old)
        assert w.save() == want
        w.close()
    assert outs[0] == outs[1] == outs[2] == outs[3]


@pytest.mark.parametrize("flags", [0, bg.GGRS_WORLD_NO_GROUPS, bg.GGRS_WORLD_UNFUSED])
def test_async_enqueue_collect_matches_sync(flags):
    """ggrs_hip_enqueue_requests / ggrs_hip_collect_checksums: same checksums and state as the
    synchronous call, batches collected oldest-first, sync calls refused while batches are pending
    (request-group worlds and one-launch-per-request worlds alike)."""
    n = 3000
    vel, ttl = cm.synthetic_particles(n, ttl="despawn")
    out = []
    for mode in ("sync", "async"):
        w = bg.World(n + 2000, max_depth=9, flags=flags)
        ids = cm.build_particles(w, with_spawn=True, ttl_init=30)
        cm.spawn_particles(w, ids, n, vel, ttl)
        w.set_depth(9)
        w.set_synctest_check_distance(4)
        fn = cm.frame_spawn_fn(50)
        cs = []
        lists = []
        F = 0
        for t in range(14):
            reqs = []
            if F > 4:
                reqs.append(bg.LoadGameState(F - 4))
                for i in range(4):
                    if i: reqs.append(bg.SaveGameState(F - 4 + i))
                    f = F - 4 + i
                    a = bg.AdvanceFrame((cm.INPUT_SPAWN if f % 3 == 1 else 0,))
                    if f % 3 == 1: a.spawn_vx, a.spawn_vy = fn(f)
                    reqs.append(a)
            reqs.append(bg.SaveGameState(F))
            a = bg.AdvanceFrame((cm.INPUT_SPAWN if F % 3 == 1 else 0,))
            if F % 3 == 1: a.spawn_vx, a.spawn_vy = fn(F)
            reqs.append(a)
            F += 1
            lists.append(reqs)
        if mode == "sync":
            for reqs in lists: cs.append(w.handle_requests(reqs))
        else:
            counts = []
            for k, reqs in enumerate(lists):
                counts.append(w.enqueue_requests(reqs))
                if k >= 2:                                   # keep three batches in flight
                    cs.append(w.collect_checksums())
            assert w.pending_batches() == 2
            with pytest.raises(bg.GgrsHipError):
                w.save()                                     # synchronous call while batches are pending
            while w.pending_batches():
                cs.append(w.collect_checksums())
            assert [len(c) for c in cs] == counts
            with pytest.raises(bg.GgrsHipError):
                w.collect_checksums()                        # nothing left
        out.append((cs, cm.snapshot_state(w, ids)))
    assert out[0][0] == out[1][0]
    cm.assert_states_equal(out[0][1], out[1][1], "async")


@pytest.mark.parametrize("n,ticks,flags", [(100_000, 40, 0), (100_000, 16, bg.GGRS_WORLD_NO_GROUPS), (3000, 80, 0)])
def test_p2p_shaped_rollbacks_100k(n, ticks, flags):
    """BASELINE config 4: 2-player p2p session shape, 100k entities, rollbacks of 0..7 frames per tick (120 ms RTT),
    confirmed frame trailing by 8; spawns and Ttl despawns inside the rolled-back window."""
    from test_oracle_selfcheck import _p2p_run
    g, o = _pair(n + 40 * (ticks + 10) + 64, 8, flags)
    a, sa = _p2p_run(g, n, ticks)
    b, sb = _p2p_run(o, n, ticks)
    assert a.depths == b.depths and len(a.all_checksums) == len(b.all_checksums) > ticks
    for (fa, ca), (fb, cb) in zip(a.all_checksums, b.all_checksums):
        assert fa == fb and ca == cb, f"frame {fa}: gpu {ca:#x} oracle {cb:#x}"
    cm.assert_states_equal(sa, sb, "p2p shape")
    assert not a.world.has_snapshot(0) and a.world.has_snapshot(a.frame - 1) and a.world.snapshot_count() <= 8
    assert a.world.snapshot_count() == b.world.snapshot_count()


def test_column_transfers_across_tile_boundaries():
    """Word columns are tile-major on the device (8192-slot layout tiles): uploads, downloads and
    spawns of arbitrary [first, first + count) ranges are a head piece + a pitched 2-D copy + a tail piece.  Every
    range must round-trip and leave its neighbours alone -- 4- and 8-byte words, rollback and live-only columns."""
    cap = 20000
    w = bg.World(cap, max_depth=4)
    A = w.register_component("A", 4, 3)
    B = w.register_component("B", 8, 2)
    N = w.register_component("N", 4, 1, rollback=False)
    w.spawn(cap, {A: None, B: None, N: None})
    rng = np.random.default_rng(3)
    shadow = {(A, k): np.zeros(cap, np.uint32) for k in range(3)}
    shadow.update({(B, k): np.zeros(cap, np.uint64) for k in range(2)})
    shadow[(N, 0)] = np.zeros(cap, np.uint32)
    ranges = [(0, 1), (1023, 2), (1000, 3000), (1024, 1024), (1, 4998), (2047, 1), (2048, 2952), (4999, 1), (0, 5000), (3071, 1026),
              (8191, 2), (8192, 8192), (8000, 400), (1, 19999), (16383, 3617), (0, 20000), (16384, 1), (8190, 8196)]
    for i, (first, count) in enumerate(ranges):
        for (c, k), sh in shadow.items():
            data = rng.integers(0, 2 ** 32 - 1, count).astype(sh.dtype) + (np.uint64(i) << np.uint64(40) if sh.dtype == np.uint64 else 0)
            data = data.astype(sh.dtype)
            w.upload_word(c, k, first, data)
            sh[first:first + count] = data
        for (c, k), sh in shadow.items():
            assert np.array_equal(w.download_word(c, k, 0, cap), sh), (c, k, first, count)
            f2, n2 = ranges[(i + 3) % len(ranges)]
            assert np.array_equal(w.download_word(c, k, f2, n2), sh[f2:f2 + n2]), (c, k, f2, n2)
    # a snapshot round trip keeps the rollback columns, and insert_component lands on the right slot of the right tile
    w.save()
    w.insert_component(A, 2049, np.array([7, 8, 9], np.uint32))
    assert [int(w.download_word(A, k, 2049, 1)[0]) for k in range(3)] == [7, 8, 9]
    assert int(w.download_word(A, 0, 2048, 1)[0]) == int(shadow[(A, 0)][2048]) and int(w.download_word(A, 0, 2050, 1)[0]) == int(shadow[(A, 0)][2050])
    w.load(0)
    for (c, k), sh in shadow.items():
        assert np.array_equal(w.download_word(c, k, 0, cap), sh), ("after load", c, k)
    ptr, ts = w.column_device_ptr(A, 0)
    assert ptr and ts == 8192 * (3 * 4 + 2 * 8)                   # tile stride = bytes of all rollback words of 8192 slots
    ptr_n, ts_n = w.column_device_ptr(N, 0)
    assert ptr_n and ts_n == 8192 * 4                             # live-only column: a plain array


def test_malformed_requests_fail_before_any_bookkeeping():
    """NULL pointers with non-zero counts, > GGRS_MAX_PLAYERS inputs and unknown kinds return GGRS_E_INVALID
    (the reference would panic / not compile) and leave frame counter, ring and state untouched."""
    import ctypes as C
    from bevy_ggrs_amd import _ffi
    n = 2000
    vel, ttl = cm.synthetic_particles(n, ttl="despawn")
    w = bg.World(n + 500, max_depth=4)
    ids = cm.build_particles(w, with_spawn=True)
    cm.spawn_particles(w, ids, n, vel, ttl)
    w.handle_requests([bg.SaveGameState(0), bg.AdvanceFrame((0,))])
    before = (w.frame, w.snapshot_count(), cm.snapshot_state(w, ids))
    out = (C.c_uint64 * 8)()

    def bad(mut):
        arr = (_ffi.Request * 3)()
        arr[0].kind, arr[0].frame = _ffi.REQ_SAVE, w.frame
        arr[1].kind = _ffi.REQ_ADVANCE
        arr[2].kind, arr[2].frame = _ffi.REQ_SAVE, w.frame + 1
        keep = mut(arr)
        for fn in ("handle_requests", "enqueue_requests"):
            rc = getattr(_ffi.lib, "ggrs_hip_" + fn)(w._p, arr, 3, out if fn == "handle_requests" else None)
            assert rc == bg.GGRS_E_INVALID, (fn, rc)
        assert w.pending_batches() == 0
        return keep

    def null_inputs(arr): arr[1].n_inputs = 2
    def too_many(arr):
        ia = (C.c_uint8 * 17)(); arr[1].inputs = C.cast(ia, C.POINTER(C.c_uint8)); arr[1].n_inputs = 17; return ia
    def unknown_kind(arr): arr[2].kind = 9
    def null_spawn(arr):
        ia = (C.c_uint8 * 1)(cm.INPUT_SPAWN); arr[1].inputs = C.cast(ia, C.POINTER(C.c_uint8)); arr[1].n_inputs = 1; arr[1].spawn_count = 10; return ia
    for m in (null_inputs, too_many, unknown_kind, null_spawn):
        bad(m)
    assert (w.frame, w.snapshot_count()) == before[:2]
    cm.assert_states_equal(cm.snapshot_state(w, ids), before[2], "after rejected requests")
    # overflow-safe ranges
    with pytest.raises(bg.GgrsHipError):
        w._check(_ffi.lib.ggrs_hip_download_word(w._p, ids[0], 0, 2 ** 64 - 4, 8, C.cast(out, C.c_void_p)))
    # the world still works
    assert len(w.handle_requests([bg.SaveGameState(w.frame), bg.AdvanceFrame((0,))])) == 1


def test_particles_systems_over_live_only_components_are_rejected():
    """PARTICLES_* / TTL_DESPAWN kernels address columns with the rollback tile stride; a
    GGRS_COMP_NO_ROLLBACK component under them is refused when the world is sealed, and the failure is permanent."""
    w = bg.World(4096, max_depth=4)
    T = w.register_component("Transform", 4, 10)
    V = w.register_component("Velocity", 4, 3, rollback=False)
    w.add_system(bg.SYS_PARTICLES_UPDATE, comp=(T, V), word=(0, 0), fparam=(0.0, -200.0, 0.0))
    for _ in range(2):
        with pytest.raises(bg.GgrsHipError) as e:
            w.spawn(10, {T: None, V: None})
        assert e.value.code == bg.GGRS_E_INVALID and "not registered for rollback" in str(e.value)


@pytest.mark.parametrize("n,flags", [(30_000, 0), (700_000, 0), (3000, bg.GGRS_WORLD_NO_GROUPS)])
@pytest.mark.parametrize("per_request", [False, True])
def test_branch_lists_dead_snapshots_and_batches(n, flags, per_request, monkeypatch):
    """A request list holding several speculative branches off one snapshot ([Load(C), Adv, Save, ...] x B): every branch
    but the last leaves nothing behind but its checksums (the next Load pops its snapshots, mod.rs:210-226), so the
    library runs it checksum-only and launches identical branches together.  Must equal the oracle executing the same
    list request by request -- checksums of every branch, ring content and live state -- also when the next Load
    targets a frame INSIDE the group's saves (not dead) and when a branch spawns (never dead)."""
    if per_request:                                            # the same lists without the run-time compiler: one launch per request, nothing eliminated
        monkeypatch.setenv("GGRS_TICK_JIT", "0")
    D, B = 4, 6
    vel, ttl = cm.synthetic_particles(n, ttl="despawn")
    fn = cm.frame_spawn_fn(60)
    res = []
    for w in (bg.World(n + 4000, max_depth=D + 2, flags=flags), OracleWorld(n + 4000, D + 2, FLAT)):
        ids = cm.build_particles(w, with_spawn=True, ttl_init=20)
        cm.spawn_particles(w, ids, n, vel, ttl)
        w.set_depth(D + 1)
        w.set_confirmed(0)
        out = w.handle_requests([bg.SaveGameState(0), bg.AdvanceFrame((0,)), bg.SaveGameState(1)])
        C = 1

        def adv(frame, spawn):
            a = bg.AdvanceFrame((cm.INPUT_SPAWN if spawn else 0,))
            if spawn: a.spawn_vx, a.spawn_vy = fn(frame)
            return a
        reqs = []
        for b in range(B):
            spawning = b == 2                                   # one branch spawns on every frame: its groups are never dead
            reqs += [bg.LoadGameState(C)]
            for i in range(D):
                reqs += [adv(C + i, spawning), bg.SaveGameState(C + 1 + i)]
            reqs.append(adv(C + D, spawning))
        # a partial rollback INTO the last branch's saves: those snapshots are read, the branch before must be alive for it
        reqs += [bg.LoadGameState(C + 2), adv(C + 2, False), bg.SaveGameState(C + 3)]
        out += w.handle_requests(reqs)
        # afterwards every frame the ring still holds must be loadable and hash as saved
        tail = []
        for f in (C + 3, C + 2, C):
            w.handle_requests([bg.LoadGameState(f)])
            tail.append(w.handle_requests([bg.SaveGameState(f)])[0])
        res.append((out, tail, cm.snapshot_state(w, ids), w.snapshot_count()))
    assert res[0][0] == res[1][0]
    assert res[0][1] == res[1][1]
    assert res[0][3] == res[1][3]
    cm.assert_states_equal(res[0][2], res[1][2], "branch lists")
    nb = D                                                     # checksums per branch
    first = res[0][0][2:2 + nb]                                # after the two warm-up Saves
    assert all(res[0][0][2 + b * nb:2 + (b + 1) * nb] == first for b in (1, 3, 4, 5)) and res[0][0][2 + 2 * nb:2 + 3 * nb] != first


@pytest.mark.parametrize("n", [1000, 250, 8100])
@pytest.mark.parametrize("per_request", [False, True])
def test_dead_branches_keep_dirty_extents(n, per_request, monkeypatch):
    """a checksum-only (dead) branch writes neither its ring slots nor the live block, so it must not lower
    their dirty extents.  A spawning branch first grows the live world past a 256- / 1024- / 8192-slot boundary, dead branches
    follow off the OLD confirmed frame, the last branch is alive, and then spawns grow len back across the boundary: stale
    liveness bits left above the lowered extent would come back as ghost entities (wrong count, wrong checksum)."""
    if per_request: monkeypatch.setenv("GGRS_TICK_JIT", "0")
    D = 4
    vel, ttl = cm.synthetic_particles(n, ttl="despawn")
    fn = cm.frame_spawn_fn(90)
    res = []
    for w in (bg.World(n + 4000, max_depth=D + 2), OracleWorld(n + 4000, D + 2, FLAT)):
        ids = cm.build_particles(w, with_spawn=True, ttl_init=50)
        cm.spawn_particles(w, ids, n, vel, ttl)
        w.set_depth(D + 1)
        w.set_confirmed(0)
        out = w.handle_requests([bg.SaveGameState(0), bg.AdvanceFrame((0,)), bg.SaveGameState(1)])
        C = 1

        def adv(frame, spawn):
            a = bg.AdvanceFrame((cm.INPUT_SPAWN if spawn else 0,))
            if spawn: a.spawn_vx, a.spawn_vy = fn(frame)
            return a

        def branch(spawning):
            r = [bg.LoadGameState(C)]
            for i in range(D):
                r += [adv(C + i, spawning), bg.SaveGameState(C + 1 + i)]
            return r + [adv(C + D, spawning)]
        # spawning branch (alive: 5 x 90 new slots), three dead branches, one alive branch that rewrites the live world
        out += w.handle_requests(branch(True) + branch(False) + branch(False) + branch(False) + branch(False))
        # now grow back across the boundary, one frame at a time, checksumming every frame
        for i in range(3):
            out += w.handle_requests([adv(C + D + 1 + i, True), bg.SaveGameState(C + D + 2 + i)])
        # and once more through dead branches off the newest snapshot
        C2 = C + D + 4
        more = []
        for b in range(3):
            more += [bg.LoadGameState(C2), adv(C2, b == 0), bg.SaveGameState(C2 + 1), adv(C2 + 1, b == 0), bg.SaveGameState(C2 + 2), adv(C2 + 2, False)]
        out += w.handle_requests(more)
        out += w.handle_requests([bg.SaveGameState(C2 + 3)])
        res.append((out, cm.snapshot_state(w, ids), w.snapshot_count(), w.active_count()))
        w.close()
    assert res[0][0] == res[1][0]
    assert res[0][2:] == res[1][2:]
    cm.assert_states_equal(res[0][1], res[1][1], "dead branches / dirty extents")


@pytest.mark.parametrize("extra_words,n", [(5, 700_000), (9, 600_000), (12, 650_000)])
def test_big_world_with_extra_untouched_components(extra_words, n):
    """The stress_test world plus a component the schedule never touches (7 + extra_words untouched rows, which row versions store
    once per ring slot): every Save equals the oracle's and the extra columns survive rollbacks byte for byte."""
    vel, ttl = cm.synthetic_particles(n, ttl="despawn")
    rng = np.random.default_rng(17)
    extra = [rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(extra_words)]
    res = []
    for w in (bg.World(n, max_depth=9), OracleWorld(n, 9, FLAT)):
        T, V, L = cm.build_particles(w)
        X = w.register_component("Extra", 4, extra_words)
        tcols = [np.full(n, cm.f32bits(cm.TRANSFORM_DEFAULT)[k], dtype=np.uint32) for k in range(10)]
        vcols = [cm.f32bits(vel[:, 0]), cm.f32bits(vel[:, 1]), np.zeros(n, dtype=np.uint32)]
        w.spawn(n, {T: tcols, V: vcols, L: [ttl], X: extra})
        drv = cm.SyncTestDriver(w, 8, max_prediction=9)
        for _ in range(11):
            drv.tick((0,))
        res.append((drv.all_checksums, cm.snapshot_state(w, (T, V, L, X))))
        w.close()
    assert res[0][0] == res[1][0]
    cm.assert_states_equal(res[0][1], res[1][1], f"extra={extra_words}")


def test_long_pipelined_run_wraps_the_host_fold_row_ring(monkeypatch):
    """Small worlds leave their per-workgroup checksum partials in a pinned row ring and the host folds them at collect time.
    With one batch always in flight the ring never drains: 1400 pipelined depth-8 ticks at 10 k entities wrap it (~1090 ticks
    of rows fit).  Every checksum must equal the same run with the rows folded forward by the next launch
    (GGRS_FOLD_FORWARD_MIN_WGS=0: two values + two tags per Save and part in the same ring), and the first ticks the oracle's."""
    n, D, ticks = 10_000, 8, 1400
    vel, ttl = cm.synthetic_particles(n, ttl="throughput")
    out = []
    for host_fold in (True, False):
        if not host_fold: monkeypatch.setenv("GGRS_FOLD_FORWARD_MIN_WGS", "0")
        w = bg.World(n, max_depth=D + 1)
        ids = cm.build_particles(w)
        cm.spawn_particles(w, ids, n, vel, ttl)
        w.set_depth(D + 1)
        w.set_synctest_check_distance(D)
        cs = []
        F = 0
        for t in range(ticks):
            reqs = []
            if F >= D:
                reqs.append(bg.LoadGameState(F - D))
                for i in range(D):
                    if i: reqs.append(bg.SaveGameState(F - D + i))
                    reqs.append(bg.AdvanceFrame((0,)))
            reqs += [bg.SaveGameState(F), bg.AdvanceFrame((0,))]
            F += 1
            w.enqueue_requests(reqs)
            if t >= 1: cs.append(w.collect_checksums())          # one batch always in flight
        while w.pending_batches(): cs.append(w.collect_checksums())
        out.append((cs, cm.snapshot_state(w, ids)))
    assert out[0][0] == out[1][0]
    cm.assert_states_equal(out[0][1], out[1][1], "host fold vs device fold")
    o = OracleWorld(n, D + 1, FLAT)
    ids = cm.build_particles(o)
    cm.spawn_particles(o, ids, n, vel, ttl)
    o.set_depth(D + 1)
    o.set_synctest_check_distance(D)
    F = 0
    for t in range(24):
        reqs = []
        if F >= D:
            reqs.append(bg.LoadGameState(F - D))
            for i in range(D):
                if i: reqs.append(bg.SaveGameState(F - D + i))
                reqs.append(bg.AdvanceFrame((0,)))
        reqs += [bg.SaveGameState(F), bg.AdvanceFrame((0,))]
        F += 1
        assert o.handle_requests(reqs) == out[0][0][t], f"tick {t}"


@pytest.mark.parametrize("n,depth,with_spawn", [(30_000, 6, False), (70_000, 8, True), (300_000, 4, False)])
def test_blocking_calls_fold_their_own_rows(monkeypatch, n, depth, with_spawn):
    """A BLOCKING ggrs_hip_handle_requests of an HBM-sized group (here: every group, GGRS_FOLD_FORWARD_MIN_WGS=0) is ONE launch: the tile workgroups leave their
    partial rows as 16-byte {value, tag} cells, the launch's own fold workgroups read each cell until its tag is there and publish the folded values -- no
    k_gen_finalize behind the kernel.  Every Checksum(u128) of a SyncTest session and the final state against the oracle, and the launch counts of ten ticks."""
    monkeypatch.setenv("GGRS_FOLD_FORWARD_MIN_WGS", "0")
    res = []
    for w in (bg.World(n + 4000, max_depth=depth + 2), OracleWorld(n + 4000, depth + 2, FLAT)):
        ids = cm.build_particles(w, with_spawn=with_spawn, ttl_init=40)
        vel, ttl = cm.synthetic_particles(n, ttl="despawn")
        cm.spawn_particles(w, ids, n, vel, ttl)
        drv = cm.SyncTestDriver(w, depth, max_prediction=depth + 1)
        gpu = isinstance(w, bg.World)
        spawn = cm.frame_spawn_fn(30) if with_spawn else None
        inp = (lambda t: (cm.INPUT_SPAWN if (with_spawn and t % 3 == 0) else 0,))
        for t in range(depth + 4): drv.tick(inp(t), spawn_fn=spawn)
        if gpu:
            assert "fold-forward" in w.kernel_info()["checksum_fold"], w.kernel_info()
            w.profile_enable(True)
        for t in range(depth + 4, depth + 14): drv.tick(inp(t), spawn_fn=spawn)
        if gpu:
            prof = w.profile_read(); w.profile_enable(False)
            assert prof["tick"][1] == 10 and prof["checksum"][1] == 0, prof                # ten blocking ticks: ten launches, no finalize
        res.append((list(drv.all_checksums), cm.snapshot_state(w, ids)))
    assert res[0][0] == res[1][0]
    cm.assert_states_equal(res[0][1], res[1][1], "self-fold")
