"""The generated request-group kernel after its vector-ALU trims (csrc/kernel_gen.hpp: SeaHash finish constants folded into the memoised tail and the
order lane, a branch-free Ttl / liveness update, the per-component LDS xor only from lanes that have a hash)
computes what it computed: particle worlds against the CPU oracle -- every checksum, the final live state, every frame the ring holds.

The worlds are shaped to reach what the trims touch: Ttl despawns inside a tick and between two Saves of one launch; a tenth of the entities without
Velocity and a tenth without Ttl (lanes without a hash, scattered through every wave); velocity.z != 0 in every tenth wave only, so that the memoised
tail is recomputed in some waves and kept in others; n = 1000 (one partial workgroup) and 70 000, the latter also in a world of 131 072 slots -- from
96 Ki slots on the kernel folds per lane in LDS (jit_lane_fold), below it xors across the wave.  Each world runs by default, with every group shape
specialised at first sight, and with deferred Saves and value tags forced."""
import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
from oracle.binding import FLAT, OracleWorld

pytestmark = pytest.mark.gpu

D = 7                     # SyncTest check distance
TICKS, P2P_TICKS = 24, 6
MODES = ("default", "specialised", "deferred_and_tags")


def _populate(w, n, forced=False):
    ids = cm.build_particles(w)
    if forced:                                                   # deferred Saves on every eligible list, value tags on (set where tests/test_gpu_deferred_saves.py sets them)
        assert w._lib.ggrs_dbg_set_value_tags(w._p, 1) == 0 and w._lib.ggrs_dbg_set_lazy_live(w._p, 3) == 0
    T, V, L = ids
    vel, ttl = cm.synthetic_particles(n, ttl="despawn")          # Ttl = 1 + slot % 300: entities die in every tick of the session
    slot = np.arange(n)
    vz = np.where(((slot // 64) % 10 == 3) & (slot % 2 == 1), np.float32(37.5), np.float32(0)).astype(np.float32)
    tcols = [np.full(n, cm.f32bits(cm.TRANSFORM_DEFAULT)[k], dtype=np.uint32) for k in range(10)]
    vcols = [cm.f32bits(vel[:, 0]), cm.f32bits(vel[:, 1]), cm.f32bits(vz)]
    w.spawn(n, {T: tcols, V: vcols, L: [ttl]})
    for s in range(3, n, 10): w.remove_component(V, s)            # no Velocity: neither hashed nor moved
    for s in range(7, n, 10): w.remove_component(L, s)            # no Ttl: never despawns
    return ids


def _ring_contents(w, ids, frames):
    out = {}
    for f in sorted(frames, reverse=True):                       # newest first: a rollback pops what is newer
        if not w.has_snapshot(f): continue
        w.handle_requests([bg.LoadGameState(f)])
        out[f] = cm.snapshot_state(w, ids)
    return out


def _session(w, n, forced=False):
    ids = _populate(w, n, forced)
    drv = cm.SyncTestDriver(w, D)
    for _ in range(TICKS): drv.tick((0,))
    cs = list(drv.all_checksums)
    p2p = cm.P2PShapeDriver(w, max_rollback=8, seed=5)           # rollbacks of 0..7 frames, mixed
    for _ in range(P2P_TICKS): p2p.tick()
    assert len(set(p2p.depths)) >= 3, p2p.depths
    cs += p2p.all_checksums
    live = cm.snapshot_state(w, ids)
    return cs, live, _ring_contents(w, ids, range(p2p.frame - 9, p2p.frame + 1))


_oracle = {}


def _want(n, cap):
    """The oracle's session, computed once per world shape and shared by the three modes (never modified)."""
    if (n, cap) not in _oracle:
        _oracle[(n, cap)] = _session(OracleWorld(cap, D + 2, FLAT), n)
    return _oracle[(n, cap)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,cap", [(1000, 1000), (70_000, 70_000), (70_000, 131_072)])
def test_trimmed_kernel_matches_the_oracle(n, cap, mode, monkeypatch):
    if mode == "specialised":
        monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
        monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    w = bg.World(cap, max_depth=D + 2)
    try:
        got = _session(w, n, forced=mode == "deferred_and_tags")
        want = _want(n, cap)
        assert len(got[0]) == len(want[0]) and len(got[0]) >= (D + 1) + (TICKS - D - 1) * D + P2P_TICKS      # SyncTest: one Save per tick until the window is full, then D; P2P: at least one
        assert got[0] == want[0], next((i, a, b) for i, (a, b) in enumerate(zip(got[0], want[0])) if a != b)
        cm.assert_states_equal(got[1], want[1], "live")
        assert int((~got[1]["alive"]).sum()) > n // 20, "entities died during the session"
        assert got[2].keys() == want[2].keys() and len(got[2]) >= 8
        for f in got[2]: cm.assert_states_equal(got[2][f], want[2][f], f"ring frame {f}")
        info = w.kernel_info()
        assert info["request_group_kernel"].startswith("ggrs_jit_tick"), info["request_group_kernel"]       # the generated kernel ran these groups, not the per-request ones
        if mode == "specialised":
            sk = info["specialised_kernel"]
            assert sk.startswith("ready (") and int(sk[len("ready ("):].split()[0]) >= 2, sk                # the SyncTest tick's shape and P2P shapes got copies of their own
        if mode == "deferred_and_tags":
            assert cm.deferred_counts(w)[0] > 0, info.get("deferred_saves")
            assert info["value_tags"].startswith("on"), info["value_tags"]
    finally:
        w.close()
