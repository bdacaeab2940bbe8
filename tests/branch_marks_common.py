"""Shared by the branch-step tests of worlds with live-only state (tests/test_gpu_branch_marks.py, tests/test_gpu_zfuzz_branch_marks.py, tests/test_branch_marks_text.py):
the test world on both backends, the oracle's list walk of a branch step, and the one library call that must equal it.

The world: `Health` (u32, checksummed) plus a non-rollback `Mesh` (2 words), and ONE user-written system --

    h = h >= input[0] ? h - input[0] : 0;
    if (h == 0) { if (slot & 1) e.despawn_rollback(); else e.despawn(); }

-- so odd slots defer their despawn on an unconfirmed frame (src/snapshot/despawn.rs:114-143) and even slots are freed at once (and lose `Mesh` at the next LoadWorld)."""
import ctypes as C

import numpy as np

import bevy_ggrs_amd as bg

HEALTH_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const unsigned a = f.n_inputs ? f.input[0] : 0u;
    e.u32(0) = e.u32(0) >= a ? e.u32(0) - a : 0u;
    if (e.u32(0) == 0) { if (e.slot & 1) e.despawn_rollback(); else e.despawn(); }
}
"""
# the particles world's despawn_particles (particles.rs:282-289) with the same choice between the two despawns
TTL_DEFER_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) {
    e.u64(0) -= 1;
    if (e.u64(0) == 0) { if (e.slot & 1) e.despawn_rollback(); else e.despawn(); }
}
"""


def health_twin(words, slot, f):
    a = f.input(0)[0] if f.n_inputs else 0
    h = words[0] - a if words[0] >= a else 0
    return [h], (0 if h else (2 if slot & 1 else 1))


def ttl_twin(words, slot, f):
    t = (words[0] - 1) & 0xFFFFFFFFFFFFFFFF
    return [t], (0 if t else (2 if slot & 1 else 1))


def is_oracle(world):
    return not isinstance(world, bg.World)


def build_health(world, n):
    H = world.register_component("Health", 4, 1)
    M = world.register_component("Mesh", 4, 2, rollback=False)
    world.checksum_component(H, [0])
    world.add_custom_system(health_twin if is_oracle(world) else HEALTH_SRC, [(H, 0)], name="decrease_health")
    health = (1 + (np.arange(n) % 5)).astype(np.uint32)
    mesh = [np.arange(n, dtype=np.uint32) + 1000, np.arange(n, dtype=np.uint32) * 7]
    world.spawn(n, {H: [health], M: mesh})
    return H, M


def build_particles_deferring(world, n, ttl_init, seed):
    """tests/common.py build_particles with despawn_particles written as a deferring user system, plus the built-in spawn system."""
    import common as cm
    T = world.register_component("Transform", 4, 10)
    V = world.register_component("Velocity", 4, 3)
    L = world.register_component("Ttl", 8, 1)
    world.set_component_default(T, cm.TRANSFORM_DEFAULT)
    world.checksum_component(V, [0, 1, 2])
    world.checksum_component(T, [0, 1, 2])
    world.add_system(bg.SYS_PARTICLES_UPDATE, comp=(T, V), word=(0, 0), fparam=(0.0, -200.0, 0.0))
    world.add_custom_system(ttl_twin if is_oracle(world) else TTL_DEFER_SRC, [(L, 0)], name="despawn_particles")
    world.add_system(bg.SYS_PARTICLES_SPAWN, comp=(T, V, L), iparam=(ttl_init, cm.INPUT_SPAWN))
    vel, _ = cm.synthetic_particles(n, ttl="despawn", seed=seed)
    ttl = (1 + (np.arange(n, dtype=np.uint64) % 7)).astype(np.uint64)      # short lives: every frame of a branch despawns someone
    cm.spawn_particles(world, (T, V, L), n, vel, ttl)
    return T, V, L


def branch_requests(F, row, k, save_last, T, spawn=None, saves=True, final_save=False):
    """[Load(F), (Advance, Save) ..] of one branch, its first k frames; saves=False: the Advances only (the replay of an adopted branch), final_save: then
    SaveGameState(F + k).  spawn(frame, advance_request) decorates an AdvanceFrame."""
    reqs = [bg.LoadGameState(F)]
    for i in range(k):
        a = bg.AdvanceFrame((int(row[i]),))
        if spawn is not None: spawn(F + i, a)
        reqs.append(a)
        if saves and (i < T - 1 or save_last): reqs.append(bg.SaveGameState(F + 1 + i))
    if final_save: reqs.append(bg.SaveGameState(F + k))
    return reqs


def oracle_walk(ow, prefix, F, pred, save_last, spawn=None):
    """The list form: the prefix, every branch as its own request list, and the LoadGameState(F) that leaves the world where the branches started."""
    B, T = pred.shape
    want = list(ow.handle_requests(prefix))
    for b in range(B):
        want += list(ow.handle_requests(branch_requests(F, pred[b], T, save_last, T, spawn)))
    ow.handle_requests([bg.LoadGameState(F)])
    return want


def library_step(native, gw, prefix, pred, flags, spawn_table=None, spawn_sel=None):
    """ggrs_hip_fanout_step_branches + collect: (rc, this step's Checksum(u128)s per rank as lists)."""
    from bevy_ggrs_amd import _ffi
    B, T = pred.shape
    pre, keep, _ = gw.build_requests(prefix)
    inputs = np.ascontiguousarray(pred.reshape(B, T, 1).astype(np.uint8))
    bs = _ffi.BranchStep()
    bs.prefix, bs.n_prefix, bs.n_branches, bs.n_frames, bs.n_inputs, bs.flags = pre, len(prefix), B, T, 1, flags
    bs.inputs = inputs.ctypes.data
    if spawn_table is not None:
        bs.spawn_table, bs.n_spawn_table, bs.spawn_sel = spawn_table, len(spawn_table), spawn_sel.ctypes.data
    ns = C.c_uint32(0)
    rc = _ffi.lib.ggrs_hip_fanout_step_branches(native._p, C.byref(bs), C.byref(ns))
    if rc != 0:
        return rc, (_ffi.lib.ggrs_hip_fanout_last_error(native._p) or b"").decode()
    tab = native.collect()
    return 0, [[int(p[0]) | (int(p[1]) << 64) for p in tab[r].reshape(-1, 2)] for r in range(tab.shape[0])]
