"""The "strike" world of the effect-binding tests (ggrs_hip_add_custom_system_effects), built twice: on a library world from HIP C++ source whose striker
SENDS to other entities, and on the CPU oracle (oracle.binding.OracleWorld, unchanged) from Python callbacks.

    Pos  2 x f32      Target  1 x u64: a link -- the RollbackOrdered index (slot) of another entity      Fuse  1 x u32: a countdown
    Hp  1 x u32       Flags  1 x u32       Low  1 x i32       Score  1 x u64                              the four effect columns

    order "last" (effects only)              countdown (GGRS_SYS_SAT_SUB_DESPAWN on Fuse: targets die mid-session), mover (Pos), striker LAST: own bindings Target,
                                             Pos.x, Pos.y
    order "first" (peer reads + effects)     striker FIRST (the peer rules: before every writer of Pos, before every other system that can despawn): own binding
                                             Target, PEER binding Pos.x of the target; then countdown, mover
    the striker sends    ADD of a wrapping-negative damage to Hp (some Hp start near 0: the u32 wraps), OR of 1 << (slot % 32) to Flags, MIN_I of a signed value to
                         Low, ADD of a value above 2^32 to Score; a few senders despawn themselves in the same call and still send.

On the oracle the striker is a callback that sends nothing; at the start of its pass it computes the whole pass's effects vectorised in numpy from the oracle's own
columns (the way peer_reads_common.py caches a pass), kept only for slots below the len at the start of the frame.  They are applied by callbacks registered LAST.
The oracle runs a system only for live entities that have its bound components, which is the apply rule (alive at the END of the frame, has the component) -- per
COLUMN: an entity without Hp still takes its Flags, Low and Score.  So there is one apply callback per effect column, each bound to that column alone, instead of one
callback bound to all four (which would drop every effect on an entity that lacks one of the four components).
Every pass also counts the sends it makes and the sends that land: a test asserts on the oracle side that more than half land.
(A helper module, no tests of its own.)"""
import struct

import numpy as np

import bevy_ggrs_amd as bg
from bevy_ggrs_amd.session import SyncTestSession
from oracle.binding import OracleWorld

f32 = np.float32
U32, U64 = np.uint32, np.uint64
OPS = (bg.EFFECT_ADD, bg.EFFECT_OR, bg.EFFECT_MIN_I, bg.EFFECT_ADD)          # Hp, Flags, Low, Score
IDENT = (0, 0, 0x7FFFFFFF, 0)

# binding 0 = Target, 1 = Pos.x, 2 = Pos.y; effect bindings 0..3 = Hp, Flags, Low, Score
STRIKE_SRC = r"""
// Query<(&Target, &Pos)> + a second Query<(&mut Hp, &mut Flags, &mut Low, &mut Score)> with get_mut(target)
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u64 t = e.u64(0);
    const ggrs_u32 k = (ggrs_u32)e.slot + (ggrs_u32)f.frame;
    const ggrs_u32 dmg = 1u + k % 5u + (__float_as_uint(e.f32(1)) & 3u);
    e.send_u32(t, 0, 0u - dmg);
    e.send_u32(t, 1, 1u << (ggrs_u32)(e.slot % 32ull));
    e.send_i32(t, 2, (int)(k % 200u) - 100);
    e.send_u64(t, 3, 0x100000000ull + dmg);
    if (k % 37u == 0u && e.slot % 11ull == 5ull) e.despawn();          // a sender that despawns itself in the same call still sends
}
"""
# ... with a peer read: the damage depends on the TARGET's Pos.x at the start of the frame (binding 0 = Target; peer binding 0 = Pos.x)
STRIKE_PEER_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u64 t = e.u64(0);
    const GgrsPeer p = e.peer(t);
    const ggrs_u32 k = (ggrs_u32)e.slot + (ggrs_u32)f.frame;
    const ggrs_u32 dmg = 1u + k % 5u + (p.ok() ? (__float_as_uint(p.f32(0)) & 3u) : 7u);
    e.send_u32(t, 0, 0u - dmg);
    e.send_u32(t, 1, 1u << (ggrs_u32)(e.slot % 32ull));
    e.send_i32(t, 2, (int)(k % 200u) - 100);
    e.send_u64(t, 3, 0x100000000ull + dmg);
    if (k % 37u == 0u && e.slot % 11ull == 5ull) e.despawn();          // a sender that despawns itself in the same call still sends
}
"""
# the comparison world of scripts/bench_peer_effects.py: the same arithmetic written to the striker's OWN Hp, Flags, Low and Score (bindings 3..6) -- no inbox, no
# apply launch, groups of any length
STRIKE_OWN_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u32 k = (ggrs_u32)e.slot + (ggrs_u32)f.frame;
    const ggrs_u32 dmg = 1u + k % 5u + (__float_as_uint(e.f32(1)) & 3u);
    if (e.u64(0) < (ggrs_u64)f.iparam[0]) {
        e.u32(3) = e.u32(3) + (0u - dmg);
        e.u32(4) = e.u32(4) | (1u << (ggrs_u32)(e.slot % 32ull));
        const int v = (int)(k % 200u) - 100; if (v < e.i32(5)) e.i32(5) = v;
        e.u64(6) = e.u64(6) + 0x100000000ull + dmg;
    }
}
"""
MOVE_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {           // Query<&mut Pos>
    e.f32(0) = e.f32(0) + 3.0f * f.dt;
    e.f32(1) = e.f32(1) - 2.0f * f.dt;
}
"""
CHILD_SRC = r"""
struct Child { float x, y; ggrs_u32 fuse, hp; ggrs_u64 target; };
__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64, const GgrsFrame&, const unsigned char* payload) {      // commands.spawn((Pos, Target, Fuse, Hp, Flags, Low, Score, Rollback))
    const Child* c = reinterpret_cast<const Child*>(payload);
    e.f32(0) = c->x; e.f32(1) = c->y; e.u64(2) = c->target; e.u32(3) = c->fuse; e.u32(4) = c->hp;
}
"""
CHILD_STRIDE = 24


class _Pass:
    """One system pass of the oracle world (peer_reads_common._Pass)."""

    def __init__(self):
        self.slot, self.frame = None, None

    def begin(self, slot, frame):
        new = self.slot is None or slot <= self.slot or frame != self.frame
        self.slot, self.frame = slot, frame
        return new

    def reset(self):
        """The next call begins a pass whatever its slot and frame: begin() alone takes a second pass over the SAME frame that starts at a higher slot than the
        first one ended at (`L5 A L5 A` with a host edit, or a Load, in between) for the first one's continuation."""
        self.slot, self.frame = None, None


class Effects:
    """What the striker's current pass sends: per effect column the combined value and the number of sends per target slot, for slots below n0 -- the len at the
    start of the frame.  sent / landed: totals over the session."""

    def __init__(self):
        self.n0, self.val, self.cnt, self.kill = 0, [None] * 4, None, None
        self.sent, self.landed = 0, 0


def _col(o, comp, word, n, dtype):
    return o.download_word(comp, word, 0, n).astype(dtype, copy=False)


def build_strike(w, *, order="last", with_spawn=False, fx=None):
    """Registers the strike world on `w` (a library world or the oracle); returns (Pos, Target, Fuse, Hp, Flags, Low, Score).  fx: the oracle's Effects record."""
    P = w.register_component("Pos", 4, 2)
    T = w.register_component("Target", 8, 1)
    F = w.register_component("Fuse", 4, 1)
    H = w.register_component("Hp", 4, 1)
    G = w.register_component("Flags", 4, 1)
    L = w.register_component("Low", 4, 1)
    S = w.register_component("Score", 8, 1)
    w.set_component_default(F, np.array([1000], dtype=U32))
    w.set_component_default(L, np.array([50], dtype=U32))
    for c, words in ((P, [0, 1]), (T, [0]), (F, [0]), (H, [0]), (G, [0]), (L, [0]), (S, [0])): w.checksum_component(c, words)
    peer = order == "first"
    s_binds = [(T, 0)] if peer else [(T, 0), (P, 0), (P, 1)]
    m_binds = [(P, 0), (P, 1)]
    c_binds = [(P, 0), (P, 1), (T, 0), (F, 0), (H, 0)]
    fx_cols = (H, G, L, S)
    oracle = isinstance(w, OracleWorld)
    if oracle:
        fx = fx if fx is not None else Effects()
        ps, pm = _Pass(), _Pass()

        def strike(words, slot, f):
            if ps.begin(slot, f.frame):
                n = w.len
                tg = _col(w, T, 0, n, U64)
                px = _col(w, P, 0, n, U32)
                on = w.alive_mask(n) & w.present_mask(T, n)
                if not peer: on = on & w.present_mask(P, n)                      # the striker's own bindings: the entities it runs for
                i = np.arange(n, dtype=np.int64)
                k = (i + f.frame).astype(U32)
                ok_t = tg < U64(n)
                ti = np.where(ok_t, tg, 0).astype(np.int64)
                if peer:
                    vis = w.alive_mask(n) & w.present_mask(P, n)                 # the peer view at the start of the frame (the striker is the first system)
                    extra = np.where(ok_t & vis[ti], px[ti] & U32(3), U32(7)).astype(U32)
                else:
                    extra = px & U32(3)
                dmg = (U32(1) + k % U32(5) + extra).astype(U32)
                send = on & ok_t
                t = ti[send]
                hp = np.zeros(n, dtype=U32); np.add.at(hp, t, (U32(0) - dmg[send]).astype(U32))
                fl = np.zeros(n, dtype=U32); np.bitwise_or.at(fl, t, (U32(1) << (i[send] % 32).astype(U32)).astype(U32))
                lo = np.full(n, 0x7FFFFFFF, dtype=np.int32); np.minimum.at(lo, t, (k[send] % U32(200)).astype(np.int32) - np.int32(100))
                sc = np.zeros(n, dtype=U64); np.add.at(sc, t, U64(0x100000000) + dmg[send].astype(U64))
                cnt = np.zeros(n, dtype=np.int64); np.add.at(cnt, t, 1)
                fx.n0, fx.val, fx.cnt = n, [hp.tolist(), fl.tolist(), lo.view(U32).tolist(), sc.tolist()], cnt.tolist()
                fx.kill = (((k % U32(37)) == 0) & (i % 11 == 5)).tolist()
                fx.sent += 4 * int(on.sum())                                     # (a send to a slot out of range is a send that does not land)
            return list(words), int(fx.kill[slot])

        def move(words, slot, f):
            if pm.begin(slot, f.frame):
                n = w.len
                dt = f32(f.dt)
                px = _col(w, P, 0, n, U32).view(f32); py = _col(w, P, 1, n, U32).view(f32)
                nx = (px + (f32(3.0) * dt).astype(f32)).astype(f32); ny = (py - (f32(2.0) * dt).astype(f32)).astype(f32)
                pm.out = (nx.view(U32).tolist(), ny.view(U32).tolist())
            return [pm.out[0][slot], pm.out[1][slot]], 0

        def make_apply(j):
            op = OPS[j]

            def apply(words, slot, f):
                if slot >= fx.n0 or not fx.cnt[slot]: return list(words), 0
                fx.landed += fx.cnt[slot]
                x, v = words[0], fx.val[j][slot]
                if op == bg.EFFECT_ADD: x = (x + v) & (0xFFFFFFFFFFFFFFFF if j == 3 else 0xFFFFFFFF)
                elif op == bg.EFFECT_OR: x = x | v
                else:                                                            # MIN_I on a 4-byte word
                    sx, sv = (x ^ 0x80000000) - 0x80000000, (v ^ 0x80000000) - 0x80000000
                    x = (sv if sv < sx else sx) & 0xFFFFFFFF
                return [x], 0
            return apply

        def child(words, slot, k, f, payload):
            x, y, fuse, hp, tgt = struct.unpack("<IIIIQ", bytes(payload[:CHILD_STRIDE]))
            return [x, y, tgt, fuse, hp]
        countdown = lambda: w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(F,), word=(0,), iparam=(1, 0))
        if peer: w.add_custom_system(strike, s_binds); countdown(); w.add_custom_system(move, m_binds)
        else: countdown(); w.add_custom_system(move, m_binds); w.add_custom_system(strike, s_binds)
        for j, c in enumerate(fx_cols): w.add_custom_system(make_apply(j), [(c, 0)])
        if with_spawn: w.add_spawn_system(child, bundle=(P, T, F, H, G, L, S), bindings=c_binds, payload_stride=CHILD_STRIDE)
    else:
        effects = [(c, 0, op) for c, op in zip(fx_cols, OPS)]
        countdown = lambda: w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(F,), word=(0,), iparam=(1, 0))
        if peer:
            w.add_custom_system(STRIKE_PEER_SRC, s_binds, name="striker", peers=[(P, 0)], effects=effects)
            countdown(); w.add_custom_system(MOVE_SRC, m_binds, name="mover")
        else:
            countdown(); w.add_custom_system(MOVE_SRC, m_binds, name="mover")
            w.add_custom_system(STRIKE_SRC, s_binds, name="striker", effects=effects)
        if with_spawn: w.add_spawn_system(CHILD_SRC, bundle=(P, T, F, H, G, L, S), bindings=c_binds, payload_stride=CHILD_STRIDE, name="child")
    return P, T, F, H, G, L, S


def strike_links(n):
    """Links (i * 389 + 17) % n -- they cross 64-slot units, 256-slot workgroups and (n > 8192) the layout tile --; every tenth out of range (n + 5); every
    thirteenth entity targets slot 0 (contention on one inbox word)."""
    i = np.arange(n, dtype=U64)
    link = (i * U64(389) + U64(17)) % U64(n)
    link[i % U64(13) == 0] = 0
    link[i % U64(10) == 3] = n + 5
    return link


def spawn_strike(w, ids, n, *, n_bare=0, links=None):
    """n entities, the last n_bare of them WITHOUT Hp (a send to their Hp is dropped, their Flags, Low and Score still take theirs).  A seventh has a short fuse:
    links end up pointing at slots that die mid-session (never slot 0).  A fifth starts with Hp below the first damage: the add wraps."""
    P, T, F, H, G, L, S = ids
    rng = np.random.default_rng(23)
    pos = rng.uniform(-100, 100, (n, 2)).astype(f32)
    i = np.arange(n)
    fuse = np.where(i % 7 == 3, 3 + i % 9, 1000).astype(U32)
    hp = np.where(i % 5 == 1, i % 3, 500 + i % 100).astype(U32)
    flags = np.zeros(n, dtype=U32)
    low = (40 - (i % 30)).astype(np.int32).view(U32)
    score = (i.astype(U64) << U64(33)) | U64(7)
    link = strike_links(n) if links is None else links
    m = n - n_bare
    cut = lambda a, s: np.ascontiguousarray(a[s])
    def bundle(s, with_hp):
        b = {P: [cut(pos[:, 0].view(U32), s), cut(pos[:, 1].view(U32), s)], T: [cut(link, s)], F: [cut(fuse, s)], G: [cut(flags, s)], L: [cut(low, s)], S: [cut(score, s)]}
        if with_hp: b[H] = [cut(hp, s)]
        return b
    w.spawn(m, bundle(slice(0, m), True))
    if n_bare: w.spawn(n_bare, bundle(slice(m, n), False))


def children(frame, n0):
    """The host side of the spawn system, a pure function of the frame: in every fourth frame five children that link to existing slots."""
    if frame % 4 != 1: return 0, None
    r = np.random.default_rng([6, frame])
    rec = np.zeros(5, dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("fuse", "<u4"), ("hp", "<u4"), ("target", "<u8")]))
    rec["x"] = r.uniform(-50, 50, 5); rec["y"] = r.uniform(-50, 50, 5); rec["fuse"] = 4 + r.integers(0, 40, 5); rec["hp"] = r.integers(0, 30, 5); rec["target"] = r.integers(0, n0, 5)
    return 5, rec


def spawn_patch(n0):
    def patch(frame, r):
        cnt, rec = children(frame, n0)
        if cnt: r.spawn_count, r.spawn_payload = cnt, rec
    return patch


def synctest_lists(cd, ticks, *, depth=8, patch=None, inputs=lambda t: (t & 3,)):
    """The request lists of a SyncTest session (check distance cd), which do not depend on the checksums: [Load(F - cd), Adv, (Save, Adv) x (cd - 1), Save(F), Adv] --
    every list ends on an AdvanceFrame."""
    sess = SyncTestSession(1, cd, depth, 0)
    out, cur = [], 0
    for t in range(ticks):
        for h, v in enumerate(inputs(t)): sess.add_local_input(h, v)
        reqs = sess.advance_frame()
        for r in reqs:
            if isinstance(r, bg.LoadGameState): cur = r.frame
            elif isinstance(r, bg.AdvanceFrame):
                if patch is not None: patch(cur, r)
                cur += 1
        sess.record_checksums([0] * sum(isinstance(r, bg.SaveGameState) for r in reqs))
        out.append(reqs)
    return out


def run_oracle(o, lists, cd):
    """The lists on the oracle, request by request, with the SyncTest confirm rule (schedule_systems.rs:204-220) where cd >= 0; returns [(frame, checksum)]."""
    got = []
    for reqs in lists:
        for r in reqs:
            if cd >= 0 and o.frame - cd >= 0: o.set_confirmed(o.frame - cd)
            cs = o.handle_requests([r])
            if isinstance(r, bg.SaveGameState): got.append((r.frame, cs[0]))
    return got
