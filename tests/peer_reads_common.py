"""The "follow" world of the peer-binding tests (ggrs_hip_add_custom_system_peers), built twice: on a library world from HIP C++ source, and on the CPU
oracle from Python callbacks that read the oracle's OWN live columns while they run.

    Pos     2 x f32           Target  1 x u64: a link -- the RollbackOrdered index (slot) of another entity        Vel  2 x f32        Hp  1 x u32
    A  follow      own bindings Vel.x, Vel.y, Target; PEER bindings Pos.x, Pos.y: Vel = (Pos of the target - own Pos) * gain, or Vel / 2 when the link is not ok()
    B  integrate   Pos += Vel * dt
    C  GGRS_SYS_SAT_SUB_DESPAWN on Hp, registered last

Under the seal rules (A before every writer of Pos, before every system that can despawn) the values A's peer reads return -- the start of the frame --
are what the oracle's columns hold when A's pass begins: nothing earlier in the frame wrote them or despawned anything.  The callbacks cache those columns
once per system pass (a call whose slot is not greater than the previous call's, or whose frame differs, starts a new pass) and take liveness from that cache,
because the oracle applies a despawn at once.  A whole pass is computed vectorised from the cache, so a callback is a list lookup.
(A helper module, no tests of its own.)"""
import struct

import numpy as np

import bevy_ggrs_amd as bg
from oracle.binding import OracleWorld

f32 = np.float32
GAIN = 0.75

FOLLOW_SRC = r"""
// Query<(&mut Vel, &Target)> + a second Query<&Pos> over the other entities: steer towards the target
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const GgrsPeer me = e.peer(e.slot), t = e.peer(e.u64(2));
    if (me.ok() && t.ok()) {
        e.f32(0) = (t.f32(0) - me.f32(0)) * f.fparam[0];
        e.f32(1) = (t.f32(1) - me.f32(1)) * f.fparam[0];
    } else {
        e.f32(0) = e.f32(0) * 0.5f;
        e.f32(1) = e.f32(1) * 0.5f;
    }
}
"""
# the same system with the peer reads replaced by reads of its OWN Pos (bindings 3, 4): the comparison world of scripts/bench_peer_reads.py -- same
# arithmetic, same columns stored, no view, no publish launch, groups of any length
FOLLOW_OWN_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    if (e.u64(2) < (ggrs_u64)f.iparam[0]) {
        e.f32(0) = (e.f32(4) - e.f32(3)) * f.fparam[0];
        e.f32(1) = (e.f32(3) - e.f32(4)) * f.fparam[0];
    } else {
        e.f32(0) = e.f32(0) * 0.5f;
        e.f32(1) = e.f32(1) * 0.5f;
    }
}
"""
INTEGRATE_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {           // Query<(&mut Pos, &Vel)>
    e.f32(0) = e.f32(0) + e.f32(2) * f.dt;
    e.f32(1) = e.f32(1) + e.f32(3) * f.dt;
}
"""
CHILD_SRC = r"""
struct Child { float x, y; ggrs_u32 hp, pad; ggrs_u64 target; };
__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64, const GgrsFrame&, const unsigned char* payload) {      // commands.spawn((Pos, Target, Vel, Hp, Rollback))
    const Child* c = reinterpret_cast<const Child*>(payload);
    e.f32(0) = c->x; e.f32(1) = c->y; e.u64(2) = c->target; e.u32(3) = c->hp;
}
"""
CHILD_STRIDE = 24


class _Pass:
    """One system pass of the oracle world: the columns at its start, and what the pass computes from them."""

    def __init__(self):
        self.slot, self.frame, self.out = None, None, None

    def begin(self, slot, frame):
        new = self.slot is None or slot <= self.slot or frame != self.frame
        self.slot, self.frame = slot, frame
        return new


def _col(o, comp, word, n, dtype):
    return o.download_word(comp, word, 0, n).astype(dtype, copy=False)


def build_follow(w, *, with_spawn=False):
    """Registers the follow world on `w` (a library world or the oracle); returns (Pos, Target, Vel, Hp)."""
    P = w.register_component("Pos", 4, 2)
    T = w.register_component("Target", 8, 1)
    V = w.register_component("Vel", 4, 2)
    H = w.register_component("Hp", 4, 1)
    w.set_component_default(H, np.array([1000], dtype=np.uint32))
    w.checksum_component(P, [0, 1]); w.checksum_component(T, [0]); w.checksum_component(V, [0, 1])
    a_binds, b_binds = [(V, 0), (V, 1), (T, 0)], [(P, 0), (P, 1), (V, 0), (V, 1)]
    c_binds = [(P, 0), (P, 1), (T, 0), (H, 0)]
    if isinstance(w, OracleWorld):
        pa, pb = _Pass(), _Pass()

        def follow(words, slot, f):
            if pa.begin(slot, f.frame):
                n = w.len
                px = _col(w, P, 0, n, np.uint32).view(f32); py = _col(w, P, 1, n, np.uint32).view(f32)
                vx = _col(w, V, 0, n, np.uint32).view(f32); vy = _col(w, V, 1, n, np.uint32).view(f32)
                tg = _col(w, T, 0, n, np.uint64)
                vis = w.alive_mask(n) & w.present_mask(P, n)             # alive AND every peer-bound component present, slot < len
                ok_t = tg < np.uint64(n)
                ti = np.where(ok_t, tg, 0).astype(np.int64)
                ok = vis & ok_t & vis[ti]                                # me.ok() && t.ok()
                g = f32(f.fparam[0])
                nvx = np.where(ok, (px[ti] - px) * g, vx * f32(0.5)).astype(f32)
                nvy = np.where(ok, (py[ti] - py) * g, vy * f32(0.5)).astype(f32)
                pa.out = (nvx.view(np.uint32).tolist(), nvy.view(np.uint32).tolist())
            return [pa.out[0][slot], pa.out[1][slot], words[2]], 0

        def integrate(words, slot, f):
            if pb.begin(slot, f.frame):
                n = w.len
                dt = f32(f.dt)
                px = _col(w, P, 0, n, np.uint32).view(f32); py = _col(w, P, 1, n, np.uint32).view(f32)
                vx = _col(w, V, 0, n, np.uint32).view(f32); vy = _col(w, V, 1, n, np.uint32).view(f32)
                nx = (px + (vx * dt).astype(f32)).astype(f32); ny = (py + (vy * dt).astype(f32)).astype(f32)
                pb.out = (nx.view(np.uint32).tolist(), ny.view(np.uint32).tolist())
            return [pb.out[0][slot], pb.out[1][slot], words[2], words[3]], 0

        def child(words, slot, k, f, payload):
            x, y, hp, _pad, tgt = struct.unpack("<IIIIQ", bytes(payload[:CHILD_STRIDE]))
            return [x, y, tgt, hp]
        w.add_custom_system(follow, a_binds, fparam=(GAIN,))
        w.add_custom_system(integrate, b_binds)
        w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, 0))
        if with_spawn: w.add_spawn_system(child, bundle=(P, T, V, H), bindings=c_binds, payload_stride=CHILD_STRIDE)
    else:
        w.add_custom_system(FOLLOW_SRC, a_binds, fparam=(GAIN,), name="follow", peers=[(P, 0), (P, 1)])
        w.add_custom_system(INTEGRATE_SRC, b_binds, name="integrate")
        w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, 0))
        if with_spawn: w.add_spawn_system(CHILD_SRC, bundle=(P, T, V, H), bindings=c_binds, payload_stride=CHILD_STRIDE, name="child")
    return P, T, V, H


def follow_links(n):
    """Links (i * 389 + 17) % n -- they cross 64-slot units, 256-slot workgroups and (n > 8192) the layout tile --; a tenth point at n + 5, out of range."""
    i = np.arange(n, dtype=np.uint64)
    link = (i * np.uint64(389) + np.uint64(17)) % np.uint64(n)
    link[i % np.uint64(10) == 3] = n + 5
    return link


def spawn_follow(w, ids, n, *, n_bare=0, links=None):
    """n entities with every component, the last n_bare of them WITHOUT Pos (not visible to a peer read; A still runs for them).  A seventh of the
    entities has a short countdown: links end up pointing at slots that die mid-session."""
    P, T, V, H = ids
    rng = np.random.default_rng(11)
    pos = rng.uniform(-100, 100, (n, 2)).astype(f32); vel = rng.uniform(-3, 3, (n, 2)).astype(f32)
    i = np.arange(n)
    hp = np.where(i % 7 == 0, 3 + i % 9, 1000).astype(np.uint32)
    link = follow_links(n) if links is None else links
    m = n - n_bare
    cols = lambda a, s: [np.ascontiguousarray(x[s]) for x in a]
    full = slice(0, m)
    w.spawn(m, {P: cols([pos[:, 0].view(np.uint32), pos[:, 1].view(np.uint32)], full), T: [np.ascontiguousarray(link[full])],
                V: cols([vel[:, 0].view(np.uint32), vel[:, 1].view(np.uint32)], full), H: [np.ascontiguousarray(hp[full])]})
    if n_bare:
        bare = slice(m, n)
        w.spawn(n_bare, {T: [np.ascontiguousarray(link[bare])], V: cols([vel[:, 0].view(np.uint32), vel[:, 1].view(np.uint32)], bare), H: [np.ascontiguousarray(hp[bare])]})


def children(frame, n0):
    """The host side of the spawn system, a pure function of the frame: in every fourth frame five children that link to existing slots."""
    if frame % 4 != 1: return 0, None
    r = np.random.default_rng([5, frame])
    rec = np.zeros(5, dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("hp", "<u4"), ("pad", "<u4"), ("target", "<u8")]))
    rec["x"] = r.uniform(-50, 50, 5); rec["y"] = r.uniform(-50, 50, 5); rec["hp"] = 4 + r.integers(0, 40, 5); rec["target"] = r.integers(0, n0, 5)
    return 5, rec


def spawn_patch(n0):
    def patch(frame, r):
        cnt, rec = children(frame, n0)
        if cnt: r.spawn_count, r.spawn_payload = cnt, rec
    return patch
