"""The "brand" world of the value-binding tests (ggrs_hip_add_custom_system_values: a user-written system inserts a component into ANOTHER entity with ITS OWN words --
e.val_*(j, k) / e.send_value(slot, j); the last sender in schedule order wins, as one value), built twice: on a library world from HIP C++ source, and on the CPU
oracle (oracle.binding.OracleWorld, unchanged) from Python callbacks.

    Hp  1 x u32      Target  1 x u64: a link -- the RollbackOrdered index (slot) of another entity      Power  1 x u32                on every entity
    Burn {dps: f32, ticks: u32, source: u32}  3 x 4 bytes, absent at spawn, registered default {1.5, 3, 0xFFFFFFFF}
    Mark {id: u64}                            absent at spawn, registered default 7

    countdown  own binding Hp, command binding Burn with CMD_REMOVE: hp += input; a burning entity counts its ticks down and loses Burn at 1 (the own-entity idiom of 3.7)
    torch      own bindings Target, Power; VALUE bindings 0 and 1, both Burn -- onto Target and onto (Target + 1) % n, dps from Power, source = own slot, ticks from
               slot + frame --; remote binding 0 = Burn (INSERT | REMOVE): a default insert onto Target and a remove onto (Target + 2) % n from other conditions.  A few torches despawn themselves
               in the same call.  (effect variant: also an effect binding ADD on Hp -- the world then takes the fused k_apply_remote_effects)
    tagger     registered AFTER torch: own bindings Target, Power; VALUE bindings 0 = Mark, 1 = Burn (two systems put values on one component: ordinals decide);
               remote binding 0 = the entity (DESPAWN), onto (Target + 2) % n
    child      (variant) a host-decided spawn system: bundle Hp, Target, Power

The world-wide ordinals g of the value bindings: torch 0 and 1 (Burn), tagger 2 (Mark) and 3 (Burn).  key = (g + 1) << 40 | (sender slot + 1).

On the oracle torch and tagger are callbacks that command nothing.  At the start of torch's pass ONE vectorised numpy pass computes every command of the frame from
the oracle's own columns -- neither Target nor Power changes in a frame, and the tagger runs for the entities torch did not despawn --, kept only for targets below the
len at the start of the frame; the winners are np.maximum.at over the keys.  ONE apply callback registered LAST and bound to Target -- which every entity has -- does
the applying: the oracle runs it for live entities only, which is the drop rule; it returns `kill` for a despawned target and otherwise calls remove_component /
insert_component: remove wins over any insert, a value wins over a default insert, the winner's words come from the winner alone.
Every pass counts what it sends and what lands (Stats): the coverage floors of test_remote_values_text.py are asserted on these.
(A helper module, no tests of its own.)"""
import numpy as np

import bevy_ggrs_amd as bg
from oracle.binding import OracleWorld
from peer_effects_common import _Pass, run_oracle, strike_links, synctest_lists  # noqa: F401  (re-exported: what the tests share)

U32, U64, F32 = np.uint32, np.uint64, np.float32
M32 = 0xFFFFFFFF
BURN_DEFAULT = (int(np.array([1.5], dtype=F32).view(U32)[0]), 3, 0xFFFFFFFF)
MARK_DEFAULT = 7
G_TORCH0, G_TORCH1, G_TAG_MARK, G_TAG_BURN = 0, 1, 2, 3

# binding 0 = Hp; command binding 0 = Burn {dps, ticks, source} with CMD_REMOVE
COUNTDOWN_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    e.u32(0) = e.u32(0) + (ggrs_u32)f.input[0];
    if (e.has(0)) {
        if (e.opt_u32(0, 1) <= 1u) e.remove(0);
        else e.opt_u32(0, 1) -= 1u;
    }
}
"""
# bindings 0 = Target, 1 = Power; value bindings 0, 1 = Burn; remote binding 0 = Burn (INSERT | REMOVE); iparam[0] = n
TORCH_BODY = r"""
    const ggrs_u64 t = e.u64(0), n = (ggrs_u64)f.iparam[0];
    const ggrs_u32 k = (ggrs_u32)e.slot + (ggrs_u32)f.frame;
    if (k % 3u == 0u) {                                                  // commands.entity(t).insert(Burn { dps: power / 2, ticks, source: me })
        e.val_f32(0, 0) = (float)e.u32(1) * 0.5f; e.val_u32(0, 1) = 2u + k % 5u; e.val_u32(0, 2) = (ggrs_u32)e.slot;
        e.send_value(t, 0);
    }
    if (k % 4u == 1u) {                                                  // ... and the neighbour of the target: a second binding of the same component; ticks stay the default
        e.val_f32(1, 0) = (float)e.u32(1) * 0.25f; e.val_u32(1, 2) = (ggrs_u32)e.slot;
        e.send_value((t + 1ull) % n, 1);
    }
    if (k % 5u == 2u) e.send_insert(t, 0);
    if (k % 7u == 3u) e.send_remove((t + 2ull) % n, 0);                 // (two past the target: where EVERY entity targets slot 0, slot 0 is not stripped in every frame)
    if (k % 37u == 0u && e.slot % 11ull == 5ull) e.despawn();          // a sender that despawns itself in the same call still sends
"""
TORCH_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {" + TORCH_BODY + "}\n"
TORCH_FX_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {" + TORCH_BODY + "    if (k % 3u == 0u) e.send_u32(t, 0, 1u + k % 4u);\n}\n"
# bindings 0 = Target, 1 = Power; value bindings 0 = Mark, 1 = Burn; remote binding 0 = the entity (DESPAWN); iparam[0] = n
TAGGER_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u64 t = e.u64(0), n = (ggrs_u64)f.iparam[0];
    const ggrs_u32 k = (ggrs_u32)e.slot + (ggrs_u32)f.frame;
    if (k % 4u == 2u) { e.val_u64(0, 0) = ((ggrs_u64)e.u32(1) << 32) | (ggrs_u64)(ggrs_u32)e.slot; e.send_value(t, 0); }
    if (k % 6u == 0u) { e.val_f32(1, 0) = (float)e.u32(1) * 2.0f; e.val_u32(1, 1) = 9u; e.val_u32(1, 2) = (ggrs_u32)e.slot; e.send_value(t, 1); }
    if (k % 61u == 17u) e.send_despawn((t + 2ull) % n);                 // (two past the target, as torch's remove)
}
"""
# the same world with the parent's feature only (the launch-count comparison, the bench's reference): every value send is a send_insert of the default
TORCH_INSERT_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u64 t = e.u64(0), n = (ggrs_u64)f.iparam[0];
    const ggrs_u32 k = (ggrs_u32)e.slot + (ggrs_u32)f.frame;
    if (k % 3u == 0u) e.send_insert(t, 0);
    if (k % 4u == 1u) e.send_insert((t + 1ull) % n, 0);
    if (k % 5u == 2u) e.send_insert(t, 0);
    if (k % 7u == 3u) e.send_remove((t + 2ull) % n, 0);
    if (k % 37u == 0u && e.slot % 11ull == 5ull) e.despawn();
}
"""
TAGGER_INSERT_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u64 t = e.u64(0), n = (ggrs_u64)f.iparam[0];
    const ggrs_u32 k = (ggrs_u32)e.slot + (ggrs_u32)f.frame;
    if (k % 4u == 2u) e.send_insert(t, 0);
    if (k % 6u == 0u) e.send_insert(t, 1);
    if (k % 61u == 17u) e.send_despawn((t + 2ull) % n);
}
"""
CHILD_SRC = r"""
struct Child { ggrs_u32 hp, power; ggrs_u64 target; };
__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64, const GgrsFrame&, const unsigned char* payload) {      // commands.spawn((Hp, Target, Power, Rollback))
    const Child* c = reinterpret_cast<const Child*>(payload);
    e.u32(0) = c->hp; e.u64(1) = c->target; e.u32(2) = c->power;
}
"""
CHILD_STRIDE = 16
CHILD_DT = np.dtype([("hp", "<u4"), ("power", "<u4"), ("target", "<u8")])


class Stats:
    """What the oracle's torches and taggers sent and what became of it, over a session (every simulated frame counts, re-simulated ones too)."""
    NAMES = ("val_absent", "val_present", "multi_same_binding", "multi_two_bindings_one_system", "multi_two_systems", "value_and_default", "value_and_remove",
             "value_and_despawn", "out_of_range", "dead_target", "spawned_this_frame", "dead_sender", "winner_differs_from_every_loser")

    def __init__(self):
        for k in self.NAMES: setattr(self, k, 0)
        self.sent = self.landed = self.frames = 0

    def floors(self):
        return {k: getattr(self, k) for k in self.NAMES}


class _Cmds:
    """The commands of the current frame, per target slot below n0 (the len at the start of the frame)."""

    def __init__(self):
        self.n0 = 0
        self.pending = None                                                         # (frame, n0, [out-of-range targets of value sends]) of the previous pass


def _countdown_fn(o, B):
    c = _Pass()

    def countdown(words, slot, f):
        if c.begin(slot, f.frame):
            n = o.len
            c.has = o.present_mask(B, n).tolist(); c.ticks = o.download_word(B, 1, 0, n).tolist()
        hp = (words[0] + f.input(0)[0]) & M32
        if c.has[slot]:
            if c.ticks[slot] <= 1: o.remove_component(B, slot)
            else: o.upload_word(B, 1, slot, np.array([c.ticks[slot] - 1], dtype=U32))
        return [hp], 0
    countdown.pass_ = c
    return countdown


def _f32_bits(x):
    return np.asarray(x, dtype=F32).view(U32)


def build_brand(w, n, *, with_spawn=False, effects=False, values=True, st=None, host_apply=False):
    """Registers the brand world on `w` (a library world or the oracle) for n entities at spawn; returns the component ids (Hp, Target, Power, Burn, Mark).
    st: the oracle's Stats.  values=False (library worlds): torch and tagger use send_insert of the default only -- the parent's feature.  host_apply (the oracle):
    `apply` is NOT registered as a system -- it would run only for entities that have Target (and Hp) --; the driver calls w.land() behind every AdvanceFrame
    instead, which runs it by host calls for every entity alive at the end of the frame, and lands the effect where the entity has Hp (tests/fuzz_user_worlds.py)."""
    H = w.register_component("Hp", 4, 1)
    T = w.register_component("Target", 8, 1)
    P = w.register_component("Power", 4, 1)
    B = w.register_component("Burn", 4, 3)
    M = w.register_component("Mark", 8, 1)
    ids = (H, T, P, B, M)
    w.set_component_default(B, np.array(BURN_DEFAULT, dtype=U32))
    w.set_component_default(M, np.array([MARK_DEFAULT], dtype=U64))
    for c, words in ((H, [0]), (T, [0]), (P, [0]), (B, [0, 1, 2]), (M, [0])): w.checksum_component(c, words)
    if isinstance(w, OracleWorld):
        st = st if st is not None else Stats()
        cm_, ps = _Cmds(), _Pass()

        def compute(f):
            n0 = w.len
            tg = w.download_word(T, 0, 0, n0).astype(U64, copy=False)
            pw = w.download_word(P, 0, 0, n0).astype(U32, copy=False)
            alive = w.alive_mask(n0)
            on = alive & w.present_mask(T, n0) & w.present_mask(P, n0)             # the entities torch runs for
            i = np.arange(n0, dtype=np.int64)
            k = (i + f.frame).astype(U32)
            kill = on & (k % U32(37) == 0) & (i % 11 == 5)
            on_tag = on & ~kill                                                    # ... and the tagger, registered after it
            tg1 = (tg + U64(1)) % U64(n)
            pf = pw.astype(F32)
            # the value sends: (ordinal, component, condition, targets, words per sender)
            burn_dflt_ticks = np.full(n0, BURN_DEFAULT[1], dtype=U32)
            sends = [
                (G_TORCH0, B, on & (k % U32(3) == 0), tg, [_f32_bits(pf * F32(0.5)), (U32(2) + k % U32(5)).astype(U32), i.astype(U32)]),
                (G_TORCH1, B, on & (k % U32(4) == 1), tg1, [_f32_bits(pf * F32(0.25)), burn_dflt_ticks, i.astype(U32)]),
                (G_TAG_MARK, M, on_tag & (k % U32(4) == 2), tg, [(pw.astype(U64) << U64(32)) | i.astype(U64)]),
                (G_TAG_BURN, B, on_tag & (k % U32(6) == 0), tg, [_f32_bits(pf * F32(2.0)), np.full(n0, 9, dtype=U32), i.astype(U32)]),
            ]
            c_ins, c_rem, c_desp = on & (k % U32(5) == 2), on & (k % U32(7) == 3), on_tag & (k % U32(61) == 17)
            c_fx = on & (k % U32(3) == 0)
            in_r = tg < U64(n0)
            ti = np.where(in_r, tg, 0).astype(np.int64)

            def per_target(c, add=None):
                a = np.zeros(n0, dtype=np.int64); np.add.at(a, ti[c & in_r], 1 if add is None else add[c & in_r]); return a
            a_ins = per_target(c_ins)
            t2 = ((tg + U64(2)) % U64(n)).astype(np.int64)                         # removes and despawns go two past the target: always in range
            a_rem = np.zeros(n0, dtype=np.int64); np.add.at(a_rem, t2[c_rem], 1)
            a_desp = np.zeros(n0, dtype=np.int64); np.add.at(a_desp, t2[c_desp], 1)
            a_fx = per_target(c_fx, (1 + k % U32(4)).astype(np.int64)) if effects else np.zeros(n0, dtype=np.int64)
            win = {B: np.zeros(n0, dtype=U64), M: np.zeros(n0, dtype=U64)}
            cnt_g = {}
            oor, n_val_sent = [], 0
            for g, comp, cond, tgt, words in sends:
                ok = cond & (tgt < U64(n0))
                tt = tgt[ok].astype(np.int64)
                np.maximum.at(win[comp], tt, (U64(g + 1) << U64(40)) | (i[ok].astype(U64) + U64(1)))
                cg = np.zeros(n0, dtype=np.int64); np.add.at(cg, tt, 1); cnt_g[g] = cg
                oor.append(tgt[cond & ~(tgt < U64(n0))].astype(np.int64))
                n_val_sent += int(cond.sum())
                st.dead_sender += int((cond & kill).sum())
                st.dead_target += int(cg[~alive].sum())
            # the previous pass's out-of-range targets that exist now were spawned in its frame: dropped as "spawned this frame"
            if cm_.pending is not None and cm_.pending[0] + 1 == f.frame and n0 > cm_.pending[1]:
                st.spawned_this_frame += int(((cm_.pending[2] >= cm_.pending[1]) & (cm_.pending[2] < n0)).sum())
            oor = np.concatenate(oor)
            cm_.pending = (f.frame, n0, oor)
            st.out_of_range += int(oor.size)
            st.frames += 1
            st.sent += n_val_sent
            # a winner whose words differ from EVERY loser's: per Burn target with >= 2 value senders, compare the winner's (dps, ticks) with each loser's
            cb = cnt_g[G_TORCH0] + cnt_g[G_TORCH1] + cnt_g[G_TAG_BURN]
            for t_ in np.nonzero((cb >= 2) & alive[:n0] & (a_desp == 0) & (a_rem == 0))[0].tolist():
                key = int(win[B][t_]); gw, sw = (key >> 40) - 1, (key & ((1 << 40) - 1)) - 1
                ww = None; losers = []
                for g, comp, cond, tgt, words in sends:
                    if comp != B: continue
                    for s_ in np.nonzero(cond & (tgt == U64(t_)))[0].tolist():
                        rec = (int(words[0][s_]), int(words[1][s_]))
                        if g == gw and s_ == sw: ww = rec
                        else: losers.append(rec)
                if ww is not None and losers and all(l != ww for l in losers): st.winner_differs_from_every_loser += 1
            cm_.n0 = n0
            cm_.kill = kill.tolist()
            cm_.ins, cm_.rem, cm_.desp, cm_.fx = a_ins.tolist(), a_rem.tolist(), a_desp.tolist(), a_fx.tolist()
            cm_.win = {B: win[B].tolist(), M: win[M].tolist()}
            cm_.cnt = {g: c.tolist() for g, c in cnt_g.items()}
            cm_.words = {g: [x.tolist() for x in words] for g, comp, cond, tgt, words in sends}
            cm_.any = ((a_ins + a_rem + a_desp + a_fx + sum(cnt_g.values())) > 0).tolist()

        def torch(words, slot, f):
            if ps.begin(slot, f.frame): compute(f)
            return list(words), int(cm_.kill[slot])

        def tagger(words, slot, f):
            return list(words), 0

        def apply(words, slot, f):
            # (runs for live entities that have Target: alive once the frame's own despawns are in)
            out = list(words)
            if slot >= cm_.n0 or not cm_.any[slot]: return out, 0
            n_ins, n_rem, n_desp = cm_.ins[slot], cm_.rem[slot], cm_.desp[slot]
            c0, c1, cm, c3 = (cm_.cnt[g][slot] for g in (G_TORCH0, G_TORCH1, G_TAG_MARK, G_TAG_BURN))
            n_vb = c0 + c1 + c3
            st.landed += n_vb + cm
            if c0 >= 2 or c1 >= 2 or c3 >= 2 or cm >= 2: st.multi_same_binding += 1
            if c0 and c1: st.multi_two_bindings_one_system += 1
            if (c0 or c1) and c3: st.multi_two_systems += 1
            if n_vb and n_ins: st.value_and_default += 1
            if n_vb and n_rem: st.value_and_remove += 1
            if n_desp:                                                            # despawn wins over everything
                if n_vb or cm: st.value_and_despawn += 1
                return out, 1
            if n_rem:                                                             # remove wins over any insert
                if w.present_mask(B, slot + 1)[slot]: w.remove_component(B, slot)
            elif n_vb:                                                            # a value wins over a default insert; the largest key wins, as one value
                key = cm_.win[B][slot]; g, s = (key >> 40) - 1, (key & ((1 << 40) - 1)) - 1
                if w.present_mask(B, slot + 1)[slot]: st.val_present += 1
                else: st.val_absent += 1
                w.insert_component(B, slot, np.array([x[s] for x in cm_.words[g]], dtype=U32))
            elif n_ins:
                w.insert_component(B, slot, np.array(BURN_DEFAULT, dtype=U32))
            if cm:
                key = cm_.win[M][slot]; g, s = (key >> 40) - 1, (key & ((1 << 40) - 1)) - 1
                if w.present_mask(M, slot + 1)[slot]: st.val_present += 1
                else: st.val_absent += 1
                w.insert_component(M, slot, np.array([cm_.words[g][0][s]], dtype=U64))
            if effects: out[1] = (out[1] + cm_.fx[slot]) & M32                    # the effects apply to the alive bits the remote commands left
            return out, 0

        def child(words, slot, k, f, payload):
            rec = np.frombuffer(bytes(payload[:CHILD_STRIDE]), dtype=CHILD_DT)[0]
            return [int(rec["hp"]), int(rec["target"]), int(rec["power"])]
        countdown = _countdown_fn(w, B)

        def begin_frame():
            """For a driver that may advance one frame twice in a row, or advance a frame in which torch runs for nobody (tests/fuzz_user_worlds.py calls it before
            every AdvanceFrame): every pass starts anew and the command record is empty -- `apply` applies nothing unless torch runs and computes this frame's."""
            ps.reset(); countdown.pass_.reset()
            cm_.n0 = 0
        w.begin_frame = begin_frame

        def on_load():
            """Behind a LoadGameState: the previous pass belongs to another timeline, so what it sent out of range is not held against the next pass's len."""
            cm_.pending = None
        w.on_load = on_load

        def land():
            m = min(cm_.n0, w.len)
            if not m: return                                                      # torch ran for nobody: nothing was sent
            alive = w.alive_mask(m)
            has_hp = w.present_mask(H, m); hp = w.download_word(H, 0, 0, m)
            for slot in range(m):
                if not alive[slot] or not cm_.any[slot]: continue
                out, kill = apply([0, int(hp[slot])], slot, None)
                if kill: w.despawn(slot)
                elif effects and has_hp[slot]: w.upload_word(H, 0, slot, np.array([out[1]], dtype=U32))
        w.land = land
        w.add_custom_system(countdown, [(H, 0)])
        w.add_custom_system(torch, [(T, 0), (P, 0)], iparam=(n, 0))
        w.add_custom_system(tagger, [(T, 0), (P, 0)], iparam=(n, 0))
        if not host_apply: w.add_custom_system(apply, [(T, 0), (H, 0)] if effects else [(T, 0)])
        if with_spawn: w.add_spawn_system(child, bundle=(H, T, P), bindings=[(H, 0), (T, 0), (P, 0)], payload_stride=CHILD_STRIDE)
    else:
        w.add_custom_system(COUNTDOWN_SRC, [(H, 0)], name="countdown", commands=[(B, bg.CMD_REMOVE)])
        fx = [(H, 0, bg.EFFECT_ADD)] if effects else []
        if values:
            w.add_custom_system(TORCH_FX_SRC if effects else TORCH_SRC, [(T, 0), (P, 0)], iparam=(n, 0), name="torch", effects=fx,
                                remote=[(B, bg.REMOTE_INSERT | bg.REMOTE_REMOVE)], values=[B, B])
            w.add_custom_system(TAGGER_SRC, [(T, 0), (P, 0)], iparam=(n, 0), name="tagger", remote=[(bg.REMOTE_ENTITY, bg.REMOTE_DESPAWN)], values=[M, B])
        else:
            w.add_custom_system(TORCH_INSERT_SRC, [(T, 0), (P, 0)], iparam=(n, 0), name="torch", remote=[(B, bg.REMOTE_INSERT | bg.REMOTE_REMOVE)])
            w.add_custom_system(TAGGER_INSERT_SRC, [(T, 0), (P, 0)], iparam=(n, 0), name="tagger", remote=[(M, bg.REMOTE_INSERT), (B, bg.REMOTE_INSERT), (bg.REMOTE_ENTITY, bg.REMOTE_DESPAWN)])
        if with_spawn: w.add_spawn_system(CHILD_SRC, bundle=(H, T, P), bindings=[(H, 0), (T, 0), (P, 0)], payload_stride=CHILD_STRIDE, name="child")
    return ids


def all_to_zero_links(n):
    """EVERY entity targets slot 0: the worst contention on one winner word."""
    return np.zeros(n, dtype=U64)


def spawn_brand(w, ids, n, *, links=None):
    """n entities with Hp, Target and Power.  Links: strike_links -- (i * 389 + 17) % n, every 13th at slot 0 (contention on one winner word), every 10th out of
    range (n + 5: in the spawn variant that slot appears mid-session).  Power differs per entity, so two senders' dps differ."""
    H, T, P, B, M = ids
    i = np.arange(n)
    w.spawn(n, {H: [((i * 37 + 11) % 101).astype(U32)], T: [strike_links(n) if links is None else links], P: [(3 + (i * 7) % 29).astype(U32)]})


def children(frame, n0):
    """The host side of the spawn system, a pure function of the frame: in every fourth frame five children that link to existing slots."""
    if frame % 4 != 1: return 0, None
    r = np.random.default_rng([6, frame])
    rec = np.zeros(5, dtype=CHILD_DT)
    rec["hp"] = r.integers(0, 30, 5); rec["power"] = r.integers(1, 20, 5); rec["target"] = r.integers(0, n0, 5)
    return 5, rec


def spawn_patch(n0):
    def patch(frame, r):
        cnt, rec = children(frame, n0)
        if cnt: r.spawn_count, r.spawn_payload = cnt, rec
    return patch


def p2p_lists(patch=None):
    """P2P-shaped lists with rollbacks of 0..7 frames -- [Load(F - k), (Advance, Save) x (k + 1)]."""
    first = bg.AdvanceFrame((1,))
    if patch is not None: patch(0, first)
    lists = [[bg.SaveGameState(0), first, bg.SaveGameState(1)]]
    F = 1
    for k in (0, 0, 1, 2, 0, 3, 4, 0, 5, 6, 0, 7, 0, 3, 0):
        k = min(k, F)
        reqs = [bg.LoadGameState(F - k)]
        for i in range(k + 1):
            adv = bg.AdvanceFrame(((F - k + i) % 3,))
            if patch is not None: patch(F - k + i, adv)
            reqs += [adv, bg.SaveGameState(F - k + i + 1)]
        lists.append(reqs); F += 1
    return lists
