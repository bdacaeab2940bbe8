"""The worlds of the peer-index tests (ggrs_hip_register_peer_index), each built twice: on a library world from HIP C++ source, and on the CPU oracle from
Python callbacks that read the oracle's OWN columns while they run (as peer_reads_common.py does), plus the numpy restatement of the index itself.

THE INDEX (model_index): slot s is a member of bucket k iff s < len, alive, the key component present -- every peer-bound component, for a world with more --
and key[s] == k < n_buckets: `np.flatnonzero(vis & (key == k))`, ascending.  `variant` names one of three DELIBERATELY WRONG restatements that the model tests
hold every committed configuration against: "descending" (the order inside a bucket reversed), "dead" (members of dead entities kept), "clamp" (key n_buckets
and above indexed into the last bucket).

census   integer only: pins the index contents through a system.
    Key  1 x u32 (the index key)      Out  8 x u32      Hp  1 x u32
    A  census   own Out[0..8]; PEER binding Key.  With b = e.bucket(own key): Out = count, slot(0), slot(count - 1), slot(e.slot % count), slot(count) == ~0,
                an order-sensitive fold h = rotl(h, 5) ^ slot over the first min(count, 64) members; then a digest of bucket key + 1 and of bucket n_buckets
                (out of range: empty).  An entity without Key probes n_buckets.
    B  rekey    own Key, Out[5]: key = (key + (fold & 3) + 1) % M with M > n_buckets: keys leave and re-enter the range
    C  GGRS_SYS_SAT_SUB_DESPAWN on Hp, registered last

crowd    the realistic world: a broad phase.
    Pos  2 x f32      Vel  2 x f32      Cell  1 x u32 (the index key: cy * GW + cx)      Hp  1 x u32
    A  separate   own Vel; PEER bindings Pos.x, Pos.y, Cell.key.  Walks the 3 x 3 cells around its own in a fixed order, sums (me - other) * w over the members
                  other than itself as f32 IN LOOP ORDER, adds the sum to Vel
    B  integrate  Pos += Vel * dt
    C  recell     own Cell.key, Pos: the cell size is a power of two (x * inv is exact), (int)floorf, the cell clamped to the grid; a position outside the
                  field gets key n_buckets: such an entity is in no bucket
    D  GGRS_SYS_SAT_SUB_DESPAWN on Hp, registered last
(A helper module, no tests of its own.)"""
import struct

import numpy as np

import bevy_ggrs_amd as bg
from oracle.binding import OracleWorld
from peer_reads_common import INTEGRATE_SRC, _Pass, _col

f32 = np.float32
u32 = np.uint32
M32 = 0xFFFFFFFF
NONE = 0xFFFFFFFF                     # the low half of b.slot(i) beyond count()
FOLD_INIT = 0x9E3779B9
VARIANTS = ("descending", "dead", "clamp")


# ------------------------------------------------------------------------------------------------------------------------------------ the index, in numpy
def model_index(alive, present, key, length, n_buckets, variant=None):
    """(start[n_buckets + 1], slots[start[-1]]) of a state: `alive`, `present` (every peer-bound component present) and `key` cover at least `length` slots."""
    n = int(length)
    alive = np.asarray(alive[:n], dtype=bool); present = np.asarray(present[:n], dtype=bool); key = np.asarray(key[:n]).astype(np.int64)
    vis = present if variant == "dead" else (alive & present)
    if variant == "clamp": key = np.minimum(key, n_buckets - 1)
    k = np.where(vis & (key < n_buckets), key, n_buckets)
    order = np.argsort(k, kind="stable")                                  # stable: slot order inside a key
    start = np.searchsorted(k[order], np.arange(n_buckets + 1), side="left").astype(u32)
    slots = order[:int(start[-1])].astype(u32)
    if variant == "descending":
        for b in range(n_buckets):
            if start[b + 1] - start[b] > 1: slots[start[b]:start[b + 1]] = slots[start[b]:start[b + 1]][::-1]
    return start, slots


def model_index_plain(alive, present, key, length, n_buckets):
    """The same by the definition, bucket by bucket (small n_buckets only)."""
    n = int(length)
    vis = np.asarray(alive[:n], dtype=bool) & np.asarray(present[:n], dtype=bool)
    key = np.asarray(key[:n])
    members = [np.flatnonzero(vis & (key == k)) for k in range(n_buckets)]
    start = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(u32)
    return start, (np.concatenate(members) if members else np.zeros(0)).astype(u32)


def _rotl(x, r):
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & np.uint64(M32)


def bucket_stats(start, slots, n_buckets):
    """Per bucket 0 .. n_buckets - 1, then one EMPTY entry at n_buckets (what every key out of range sees): count, slot(0), slot(count - 1), fold, digest."""
    cnt = np.concatenate([np.diff(start.astype(np.int64)), [0]])
    st = np.concatenate([start[:-1].astype(np.int64), [0]])
    pad = np.concatenate([slots.astype(np.int64), [0]])                   # (an index that is never used by an empty bucket)
    has = cnt > 0
    first = np.where(has, pad[np.minimum(st, len(slots))], NONE).astype(np.uint64)
    last = np.where(has, pad[np.minimum(st + np.maximum(cnt, 1) - 1, len(slots))], NONE).astype(np.uint64)
    h = np.full(n_buckets + 1, FOLD_INIT, dtype=np.uint64)
    for i in range(int(min(64, cnt.max(initial=0)))):
        m = cnt > i
        h = np.where(m, _rotl(h, 5) ^ pad[np.minimum(st + i, len(slots))].astype(np.uint64), h)
    digest = h ^ ((cnt.astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(M32)) ^ _rotl(first, 7) ^ _rotl(last, 13)
    return cnt, st, first, last, h, digest


# ------------------------------------------------------------------------------------------------------------------------------------ census
CENSUS_SRC = r"""
// Query<&mut Out> + the peer index over Key: what does the index say about my bucket, the next one, and one out of range
__device__ ggrs_u32 census_rotl(ggrs_u32 x, int r) { return (x << r) | (x >> (32 - r)); }
__device__ ggrs_u32 census_fold(const GgrsBucket& b) {
    ggrs_u32 h = 0x9E3779B9u;
    const ggrs_u32 n = b.count() < 64u ? b.count() : 64u;
    for (ggrs_u32 i = 0; i < n; ++i) h = census_rotl(h, 5) ^ (ggrs_u32)b.slot(i);
    return h;
}
__device__ ggrs_u32 census_digest(const GgrsBucket& b) {
    return census_fold(b) ^ (b.count() * 0x9E3779B1u) ^ census_rotl((ggrs_u32)b.slot(0u), 7) ^ census_rotl((ggrs_u32)b.slot(b.count() - 1u), 13);
}
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u32 nb = (ggrs_u32)f.iparam[0];
    const GgrsPeer me = e.peer(e.slot);
    const ggrs_u32 key = me.ok() ? me.u32(0) : nb;
    const GgrsBucket b = e.bucket(key);
    const ggrs_u32 n = b.count();
    e.u32(0) = n;
    e.u32(1) = (ggrs_u32)b.slot(0u);
    e.u32(2) = (ggrs_u32)b.slot(n - 1u);
    e.u32(3) = (ggrs_u32)b.slot(n ? (ggrs_u32)(e.slot % n) : 0u);
    e.u32(4) = b.slot(n) == ~0ull ? 1u : 0u;
    e.u32(5) = census_fold(b);
    e.u32(6) = census_digest(e.bucket(key + 1u));
    e.u32(7) = census_digest(e.bucket(nb));
}
"""
REKEY_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {           // Query<(&mut Key, &Out)>
    e.u32(0) = (e.u32(0) + (e.u32(1) & 3u) + 1u) % (ggrs_u32)f.iparam[0];
}
"""
CENSUS_CHILD_SRC = r"""
struct Child { ggrs_u32 key, hp; };
__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64, const GgrsFrame&, const unsigned char* payload) {      // commands.spawn((Key, Out, Hp, Rollback))
    const Child* c = reinterpret_cast<const Child*>(payload);
    e.u32(0) = c->key; e.u32(1) = c->hp;
}
"""
CENSUS_CHILD_STRIDE = 8


def census_modulus(nb):
    return nb + max(1, nb // 4) + 1


def census_pass_out(alive, present, key, length, nb, variant=None):
    """What system A writes for every slot below `length` (rows: the 8 Out words), from the columns at the start of its pass."""
    n = int(length)
    start, slots = model_index(alive, present, key, n, nb, variant)
    cnt, st, first, last, fold, digest = bucket_stats(start, slots, nb)
    s = np.arange(n, dtype=np.int64)
    ok = np.asarray(alive[:n], dtype=bool) & np.asarray(present[:n], dtype=bool)           # me.ok(): the true rule, whatever the variant did to the index
    kraw = np.where(ok, np.asarray(key[:n]).astype(np.int64), nb)
    k0 = np.where(kraw < nb, kraw, nb)
    k1 = (kraw + 1) & M32; k1 = np.where(k1 < nb, k1, nb)
    pad = np.concatenate([slots.astype(np.int64), [0]])
    c0 = cnt[k0]
    pick = np.where(c0 > 0, pad[np.minimum(st[k0] + s % np.maximum(c0, 1), len(slots))], NONE)
    out = np.stack([c0, first[k0].astype(np.int64), last[k0].astype(np.int64), pick, np.ones(n, dtype=np.int64), fold[k0].astype(np.int64),
                    digest[k1].astype(np.int64), np.full(n, int(digest[nb]), dtype=np.int64)], axis=1)
    return out.astype(np.uint64)


def build_census(w, nb, *, with_spawn=False, variant=None):
    """Registers the census world on `w` (a library world or the oracle); returns (Key, Out, Hp).  `variant`: a wrong index restatement, oracle only."""
    K = w.register_component("Key", 4, 1)
    O = w.register_component("Out", 4, 8)
    H = w.register_component("Hp", 4, 1)
    w.set_component_default(H, np.array([1000], dtype=u32))
    w.checksum_component(K, [0]); w.checksum_component(O, list(range(8)))
    a_binds, b_binds, c_binds = [(O, k) for k in range(8)], [(K, 0), (O, 5)], [(K, 0), (H, 0)]
    M = census_modulus(nb)
    if isinstance(w, OracleWorld):
        pa = _Pass()

        def census(words, slot, f):
            if pa.begin(slot, f.frame):
                n = w.len
                pa.out = census_pass_out(w.alive_mask(n), w.present_mask(K, n), _col(w, K, 0, n, u32), n, nb, variant).tolist()
            return pa.out[slot], 0

        def rekey(words, slot, f):
            return [((words[0] + (words[1] & 3) + 1) & M32) % M, words[1]], 0

        def child(words, slot, k, f, payload):
            key, hp = struct.unpack("<II", bytes(payload[:CENSUS_CHILD_STRIDE]))
            return [key, hp]
        w.add_custom_system(census, a_binds, iparam=(nb,))
        w.add_custom_system(rekey, b_binds, iparam=(M,))
        w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, 0))
        if with_spawn: w.add_spawn_system(child, bundle=(K, O, H), bindings=c_binds, payload_stride=CENSUS_CHILD_STRIDE)
    else:
        w.register_peer_index(K, 0, nb)
        w.add_custom_system(CENSUS_SRC, a_binds, iparam=(nb,), name="census", peers=[(K, 0)])
        w.add_custom_system(REKEY_SRC, b_binds, iparam=(M,), name="rekey")
        w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, 0))
        if with_spawn: w.add_spawn_system(CENSUS_CHILD_SRC, bundle=(K, O, H), bindings=c_binds, payload_stride=CENSUS_CHILD_STRIDE, name="child")
    return K, O, H


def census_keys(n, nb, pattern="mixed"):
    i = np.arange(n, dtype=np.int64)
    if pattern == "one": return np.full(n, nb // 2, dtype=u32)
    if pattern == "out": return np.full(n, nb, dtype=u32)
    return ((i * 7 + i // 3) % census_modulus(nb)).astype(u32)


def spawn_census(w, ids, n, nb, *, n_bare=0, pattern="mixed"):
    """n entities, the last n_bare of them WITHOUT Key (in no bucket; A still runs for them).  A seventh has a short countdown: members die mid-session."""
    K, O, H = ids
    i = np.arange(n)
    hp = np.where(i % 7 == 0, 3 + i % 9, 1000).astype(u32)
    key = census_keys(n, nb, pattern)
    m = n - n_bare
    zeros = lambda c: [np.zeros(c, dtype=u32) for _ in range(8)]
    if m: w.spawn(m, {K: [np.ascontiguousarray(key[:m])], O: zeros(m), H: [np.ascontiguousarray(hp[:m])]})
    if n_bare: w.spawn(n_bare, {O: zeros(n_bare), H: [np.ascontiguousarray(hp[m:])]})


def census_children(frame, nb):
    """The host side of the spawn system, a pure function of the frame: in every third frame four children whose keys land in existing buckets."""
    if frame % 3 != 1: return 0, None
    r = np.random.default_rng([7, frame])
    rec = np.zeros(4, dtype=np.dtype([("key", "<u4"), ("hp", "<u4")]))
    rec["key"] = r.integers(0, nb, 4); rec["hp"] = 4 + r.integers(0, 40, 4)
    return 4, rec


def census_spawn_patch(nb):
    def patch(frame, r):
        cnt, rec = census_children(frame, nb)
        if cnt: r.spawn_count, r.spawn_payload = cnt, rec
    return patch


# ------------------------------------------------------------------------------------------------------------------------------------ crowd
SEPARATE_SRC = r"""
// Query<&mut Vel> + a second Query<(&Pos, &Cell)> over the entities of the 3 x 3 cells around mine: push away from every neighbour
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const int gw = (int)f.iparam[0], gh = (int)f.iparam[1];
    const GgrsPeer me = e.peer(e.slot);
    if (!me.ok()) return;
    const ggrs_u32 key = me.u32(2);
    if (key >= (ggrs_u32)(gw * gh)) return;                      // outside the field: in no cell
    const int cx = (int)(key % (ggrs_u32)gw), cy = (int)(key / (ggrs_u32)gw);
    const float x = me.f32(0), y = me.f32(1), w = f.fparam[0];
    float sx = 0.0f, sy = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
        const int nx = cx + dx, ny = cy + dy;
        if (nx < 0 || nx >= gw || ny < 0 || ny >= gh) continue;
        const GgrsBucket b = e.bucket((ggrs_u32)(ny * gw + nx));
        const ggrs_u32 n = b.count();
        for (ggrs_u32 i = 0; i < n; ++i) {
            const ggrs_u64 s = b.slot(i);
            if (s == e.slot) continue;
            const GgrsPeer p = e.peer(s);
            sx = sx + (x - p.f32(0)) * w;
            sy = sy + (y - p.f32(1)) * w;
        }
    }
    e.f32(0) = e.f32(0) + sx;
    e.f32(1) = e.f32(1) + sy;
}
"""
# the same arithmetic written the only way a world WITHOUT the index allows: a loop over every slot through e.peer(i) with the cell test inside
# (scripts/bench_peer_index.py measures it against SEPARATE_SRC; f.iparam[1] carries len here, the grid is square)
SEPARATE_BRUTE_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const int gw = (int)f.iparam[0], gh = gw; const ggrs_u64 len = (ggrs_u64)f.iparam[1];
    const GgrsPeer me = e.peer(e.slot);
    if (!me.ok()) return;
    const ggrs_u32 key = me.u32(2);
    if (key >= (ggrs_u32)(gw * gh)) return;
    const int cx = (int)(key % (ggrs_u32)gw), cy = (int)(key / (ggrs_u32)gw);
    const float x = me.f32(0), y = me.f32(1), w = f.fparam[0];
    float sx = 0.0f, sy = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
        const int nx = cx + dx, ny = cy + dy;
        if (nx < 0 || nx >= gw || ny < 0 || ny >= gh) continue;
        const ggrs_u32 want = (ggrs_u32)(ny * gw + nx);
        for (ggrs_u64 s = 0; s < len; ++s) {
            if (s == e.slot) continue;
            const GgrsPeer p = e.peer(s);
            if (!p.ok() || p.u32(2) != want) continue;
            sx = sx + (x - p.f32(0)) * w;
            sy = sy + (y - p.f32(1)) * w;
        }
    }
    e.f32(0) = e.f32(0) + sx;
    e.f32(1) = e.f32(1) + sy;
}
"""
RECELL_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {           // Query<(&mut Cell, &Pos)>
    const int gw = (int)f.iparam[0], gh = (int)f.iparam[1];
    const float inv = f.fparam[0], x = e.f32(1), y = e.f32(2);
    const float fx = floorf(x * inv), fy = floorf(y * inv);
    if (!(fx >= 0.0f && fx < (float)gw && fy >= 0.0f && fy < (float)gh)) { e.u32(0) = (ggrs_u32)(gw * gh); return; }   // outside the field (or not a number)
    int cx = (int)fx, cy = (int)fy;
    cx = cx < 0 ? 0 : (cx > gw - 1 ? gw - 1 : cx); cy = cy < 0 ? 0 : (cy > gh - 1 ? gh - 1 : cy);
    e.u32(0) = (ggrs_u32)(cy * gw + cx);
}
"""
CELL = f32(4.0)                        # a power of two: x * (1 / CELL) is exact
WEIGHT = f32(0.03)                     # not a power of two: every product rounds, so the order of the sum shows in its bits


def cell_of(x, y, gw, gh):
    """C's arithmetic in numpy."""
    inv = f32(1.0) / CELL
    fx = np.floor((x.astype(f32) * inv).astype(f32)); fy = np.floor((y.astype(f32) * inv).astype(f32))
    inside = (fx >= 0) & (fx < gw) & (fy >= 0) & (fy < gh)
    cx = np.clip(np.where(inside, fx, 0).astype(np.int64), 0, gw - 1); cy = np.clip(np.where(inside, fy, 0).astype(np.int64), 0, gh - 1)
    return np.where(inside, cy * gw + cx, gw * gh).astype(u32)


def separate_pass_out(alive, present, px, py, key, vx, vy, length, gw, gh, variant=None):
    """What system A writes (Vel.x, Vel.y as u32 bit patterns) for every slot below `length`: the f32 sums in loop order, one member position at a time."""
    n = int(length); nb = gw * gh
    start, slots = model_index(alive, present, key, n, nb, variant)
    start = start.astype(np.int64); pad = np.concatenate([slots.astype(np.int64), [0]])
    ok = np.asarray(alive[:n], dtype=bool) & np.asarray(present[:n], dtype=bool)
    k = np.asarray(key[:n]).astype(np.int64)
    act = ok & (k < nb)
    cx = np.where(act, k % gw, 0); cy = np.where(act, k // gw, 0)
    s = np.arange(n, dtype=np.int64)
    x = px[:n].astype(f32); y = py[:n].astype(f32)
    sx = np.zeros(n, dtype=f32); sy = np.zeros(n, dtype=f32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            nx, ny = cx + dx, cy + dy
            inb = act & (nx >= 0) & (nx < gw) & (ny >= 0) & (ny < gh)
            b = np.where(inb, ny * gw + nx, 0)
            st = start[b]; cnt = np.where(inb, start[b + 1] - st, 0)
            for i in range(int(cnt.max(initial=0))):
                m = cnt > i
                o = pad[np.where(m, st + i, len(slots))]
                m = m & (o != s)
                sx = np.where(m, (sx + ((x - x[o]).astype(f32) * WEIGHT).astype(f32)).astype(f32), sx)
                sy = np.where(m, (sy + ((y - y[o]).astype(f32) * WEIGHT).astype(f32)).astype(f32), sy)
    nvx = np.where(act, (vx[:n].astype(f32) + sx).astype(f32), vx[:n].astype(f32)).astype(f32)
    nvy = np.where(act, (vy[:n].astype(f32) + sy).astype(f32), vy[:n].astype(f32)).astype(f32)
    return nvx.view(u32), nvy.view(u32)


def build_crowd(w, gw, gh, *, variant=None, brute_len=0):
    """Registers the crowd world on `w`; returns (Pos, Vel, Cell, Hp).  brute_len != 0 (library worlds, square grids): A written without the index, a loop over
    that many slots, for the benchmark."""
    P = w.register_component("Pos", 4, 2)
    V = w.register_component("Vel", 4, 2)
    Cl = w.register_component("Cell", 4, 1)
    H = w.register_component("Hp", 4, 1)
    w.set_component_default(H, np.array([1000], dtype=u32))
    w.checksum_component(P, [0, 1]); w.checksum_component(V, [0, 1]); w.checksum_component(Cl, [0])
    a_binds, b_binds, c_binds = [(V, 0), (V, 1)], [(P, 0), (P, 1), (V, 0), (V, 1)], [(Cl, 0), (P, 0), (P, 1)]
    inv = float(f32(1.0) / CELL)
    if isinstance(w, OracleWorld):
        pa, pb, pc = _Pass(), _Pass(), _Pass()
        F = lambda c, k, n: _col(w, c, k, n, u32).view(f32)

        def separate(words, slot, f):
            if pa.begin(slot, f.frame):
                n = w.len
                vis = w.present_mask(P, n) & w.present_mask(Cl, n)
                ox, oy = separate_pass_out(w.alive_mask(n), vis, F(P, 0, n), F(P, 1, n), _col(w, Cl, 0, n, u32), F(V, 0, n), F(V, 1, n), n, gw, gh, variant)
                pa.out = (ox.tolist(), oy.tolist())
            return [pa.out[0][slot], pa.out[1][slot]], 0

        def integrate(words, slot, f):
            if pb.begin(slot, f.frame):
                n = w.len; dt = f32(f.dt)
                nx = (F(P, 0, n) + (F(V, 0, n) * dt).astype(f32)).astype(f32); ny = (F(P, 1, n) + (F(V, 1, n) * dt).astype(f32)).astype(f32)
                pb.out = (nx.view(u32).tolist(), ny.view(u32).tolist())
            return [pb.out[0][slot], pb.out[1][slot], words[2], words[3]], 0

        def recell(words, slot, f):
            if pc.begin(slot, f.frame):
                n = w.len
                pc.out = cell_of(F(P, 0, n), F(P, 1, n), gw, gh).tolist()
            return [pc.out[slot], words[1], words[2]], 0
        w.add_custom_system(separate, a_binds, iparam=(gw, gh), fparam=(float(WEIGHT),))
        w.add_custom_system(integrate, b_binds)
        w.add_custom_system(recell, c_binds, iparam=(gw, gh), fparam=(inv,))
        w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, 0))
    else:
        if not brute_len: w.register_peer_index(Cl, 0, gw * gh)
        w.add_custom_system(SEPARATE_BRUTE_SRC if brute_len else SEPARATE_SRC, a_binds, iparam=(gw, brute_len or gh), fparam=(float(WEIGHT),), name="separate", peers=[(P, 0), (P, 1), (Cl, 0)])
        w.add_custom_system(INTEGRATE_SRC, b_binds, name="integrate")
        w.add_custom_system(RECELL_SRC, c_binds, iparam=(gw, gh), fparam=(inv,), name="recell")
        w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, 0))
    return P, V, Cl, H


def crowd_positions(n, gw, gh, seed, span=None):
    """n positions inside a patch of span x span cells at the far corner of the field (so keys are large), a twentieth of them outside the field."""
    rng = np.random.default_rng([3, seed])
    span = min(gw, gh, span or max(2, int(np.sqrt(n / 3.0))))
    x0, y0 = (gw - span) * float(CELL), (gh - span) * float(CELL)
    pos = np.stack([rng.uniform(x0, x0 + span * float(CELL), n), rng.uniform(y0, y0 + span * float(CELL), n)], axis=1).astype(f32)
    out = np.arange(n) % 20 == 7
    pos[out, 0] = -pos[out, 0] - f32(1.0)
    vel = rng.uniform(-2, 2, (n, 2)).astype(f32)
    return pos, vel


def spawn_crowd(w, ids, n, gw, gh, seed=1, *, n_bare=0, span=None):
    """n entities, the last n_bare WITHOUT Cell (in no bucket and not ok() as a peer); a seventh has a short countdown."""
    P, V, Cl, H = ids
    pos, vel = crowd_positions(n, gw, gh, seed, span)
    key = cell_of(pos[:, 0], pos[:, 1], gw, gh)
    i = np.arange(n)
    hp = np.where(i % 7 == 0, 3 + i % 9, 1000).astype(u32)
    m = n - n_bare
    col = lambda a, s: np.ascontiguousarray(a[s]).view(u32)
    full = slice(0, m)
    w.spawn(m, {P: [col(pos[:, 0], full), col(pos[:, 1], full)], V: [col(vel[:, 0], full), col(vel[:, 1], full)], Cl: [np.ascontiguousarray(key[full])], H: [np.ascontiguousarray(hp[full])]})
    if n_bare:
        bare = slice(m, n)
        w.spawn(n_bare, {P: [col(pos[:, 0], bare), col(pos[:, 1], bare)], V: [col(vel[:, 0], bare), col(vel[:, 1], bare)], H: [np.ascontiguousarray(hp[bare])]})


# ------------------------------------------------------------------------------------------------------------------------------------ sessions
def census_edits(w, ids, t, n, nb):
    """Host edits between request lists, a pure function of the tick: a key uploaded out of range, the key component removed and inserted, a member despawned."""
    K, O, H = ids
    alive, has = w.alive_mask(n), w.present_mask(K, n)
    if t % 3 == 1:
        w.upload_word(K, 0, (t * 37) % n, np.array([nb + 5 if t % 2 else 0xFFFFFFF0], dtype=u32))
    s = (t // 4 * 11 + 2) % n
    if t % 4 == 2 and alive[s] and has[s]: w.remove_component(K, s)
    if t % 4 == 3 and alive[s] and not has[s]: w.insert_component(K, s, np.array([t % nb], dtype=u32))
    s = (t * 53 + 1) % n
    if t % 5 == 4 and alive[s]: w.despawn(s)


def census_session(w, n, nb, cd, ticks, *, n_bare=0, with_spawn=False, edits=False, variant=None, pattern="mixed", check=None):
    """A SyncTest session of the census world on `w`; yields after every tick the checksums so far; returns nothing else -- callers read w afterwards."""
    import common as cm
    kw = {"variant": variant} if isinstance(w, OracleWorld) else {}
    ids = build_census(w, nb, with_spawn=with_spawn, **kw)
    spawn_census(w, ids, n, nb, n_bare=n_bare, pattern=pattern)
    if edits:
        # a host edit is not part of any snapshot, so a SyncTest session would (rightly) report the re-simulated frames as mismatched: plain lists instead, every
        # third one with a rollback of `cd` frames behind it -- the Load's group builds its index from a ring slot that does not hold the later edits
        w.set_depth(8)
        if not isinstance(w, OracleWorld): w.set_synctest_check_distance(-1)
        out = []
        for t in range(ticks):
            census_edits(w, ids, t, n, nb)
            F = w.frame
            reqs = [bg.SaveGameState(F), bg.AdvanceFrame((t & 3,))]
            if t % 3 == 2 and F >= cd:
                reqs += [bg.SaveGameState(F + 1), bg.LoadGameState(F + 1 - cd)] + [r for k in range(cd) for r in (bg.AdvanceFrame((k & 3,)), bg.SaveGameState(F + 2 - cd + k))][:-1]
            saves = [r.frame for r in reqs if isinstance(r, bg.SaveGameState)]
            cs = []
            if isinstance(w, OracleWorld):
                for r in reqs: cs += w.handle_requests([r])
            else: cs = w.handle_requests(reqs)
            out += list(zip(saves, cs))
            yield out
        if check: check(w)
        return
    drv = cm.SyncTestDriver(w, cd)
    patch = census_spawn_patch(nb) if with_spawn else None
    for t in range(ticks):
        drv.tick((t & 3,), patch=patch)
        yield drv.all_checksums
    if check: check(w)


def crowd_session(w, n, gw, gh, cd, ticks, *, seed=1, n_bare=0, variant=None, span=None):
    import common as cm
    kw = {"variant": variant} if isinstance(w, OracleWorld) else {}
    ids = build_crowd(w, gw, gh, **kw)
    spawn_crowd(w, ids, n, gw, gh, seed, n_bare=n_bare, span=span)
    drv = cm.SyncTestDriver(w, cd)
    for t in range(ticks):
        drv.tick((t & 3,))
        yield drv.all_checksums


def run_all(gen):
    out = None
    for out in gen: pass
    return list(out or [])


def first_difference(gen, want):
    """Runs a session until its checksums leave `want` (the right session's): the index of the first differing Save, or None when it never happens."""
    for got in gen:
        for k, (a, b) in enumerate(zip(got, want)):
            if a != b: return k
    return None


# the committed configurations: the GPU tests run them on the device, the model tests hold the wrong restatements against every one of them on the oracle
#           name: (n, n_buckets, check distance, ticks, keyword arguments)
CENSUS_CONFIGS = {
    "65 cd2": (65, 7, 2, 8, {"n_bare": 5}),
    "65 cd7": (65, 7, 7, 11, {"n_bare": 5}),
    "600 cd2": (600, 40, 2, 8, {"n_bare": 30}),
    "600 cd7": (600, 300, 7, 11, {"n_bare": 30}),
    "8300 cd2": (8300, 255, 2, 5, {"n_bare": 100}),
    "8300 cd7": (8300, 1000, 7, 9, {"n_bare": 100}),
    "spawns": (300, 24, 2, 12, {"with_spawn": True}),
    "edits": (400, 30, 3, 14, {"edits": True, "n_bare": 10}),
}
#           name: (n, grid width, grid height, check distance, ticks, seed, span)
CROWD_CONFIGS = {
    "600 16x16": (600, 16, 16, 2, 6, 1, None),
    "8300 16x16": (8300, 16, 16, 2, 6, 2, None),
    "600 255x257": (600, 255, 257, 3, 6, 3, 12),
    "8300 255x257": (8300, 255, 257, 2, 6, 4, 40),
}
