"""The "hit" world of the remote-command tests (ggrs_hip_add_custom_system_remote: a user-written system despawns OTHER entities and inserts / removes their
components -- e.send_despawn(slot), e.send_insert(slot, j), e.send_remove(slot, j)), built twice: on a library world from HIP C++ source, and on the CPU oracle
(oracle.binding.OracleWorld, unchanged) from Python callbacks.

    Hp  1 x u32      Target  1 x u64: a link -- the RollbackOrdered index (slot) of another entity      on every entity
    Stun {ticks, seed}  2 x u32, absent at spawn, registered default {5, 77}                            Shield  1 x u64, default 0xABCD00000007, on every fourth entity
    Seen  1 x u32 (the watcher variant only)

    watcher    (variant, registered FIRST: the peer rules) own bindings Target, Seen; peer-reads Stun.ticks of its target
    countdown  own binding Hp, command binding Stun with CMD_REMOVE: hp += input; a stunned entity counts down and loses Stun at 1 (the own-entity idiom of 3.7)
    striker    registered LAST: own binding Target; remote bindings 0 = Stun (INSERT), 1 = Shield (INSERT | REMOVE), 2 = the entity (DESPAWN).  From conditions on
               slot + frame it sends insert Stun, remove Shield, insert Shield and despawn to its target; a few strikers despawn themselves in the same call
    child      (variant) a host-decided spawn system: bundle Hp, Target

On the oracle the striker is a callback that commands nothing; at the start of its pass it computes the whole pass's commands vectorised in numpy from the oracle's
own columns, kept only for slots below the len at the start of the frame.  ONE apply callback registered LAST and bound to Target -- a component every test entity has
-- does the applying: the oracle runs it for live entities only, which is the drop rule (alive once the frame's own despawns are in); it returns `kill` for a
despawned target (despawn wins over everything) and otherwise calls remove_component / insert_component with the default words (remove wins over insert).
Every pass counts what it sends and what lands (Stats): the coverage floors of test_remote_commands_text.py are asserted on these.
(A helper module, no tests of its own.)"""
import numpy as np

import bevy_ggrs_amd as bg
from oracle.binding import OracleWorld
from peer_effects_common import _Pass, run_oracle, strike_links, synctest_lists  # noqa: F401  (re-exported: what the tests share)

U32, U64 = np.uint32, np.uint64
M32 = 0xFFFFFFFF
STUN_DEFAULT = (5, 77)
SHIELD_DEFAULT = 0xABCD00000007

# binding 0 = Hp; command binding 0 = Stun {ticks, seed} with CMD_REMOVE
COUNTDOWN_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    e.u32(0) = e.u32(0) + (ggrs_u32)f.input[0];
    if (e.has(0)) {
        if (e.opt_u32(0, 0) <= 1u) e.remove(0);
        else e.opt_u32(0, 0) -= 1u;
    }
}
"""
# binding 0 = Target; remote bindings 0 = Stun (INSERT), 1 = Shield (INSERT | REMOVE), 2 = the entity (DESPAWN)
STRIKER_SRC = r"""
// Query<&Target> + Commands: commands.entity(t).insert(Stun::default()) / .remove::<Shield>() / .insert(Shield::default()) / .despawn()
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u64 t = e.u64(0);
    const ggrs_u32 k = (ggrs_u32)e.slot + (ggrs_u32)f.frame;
    if (k % 3u == 0u) e.send_insert(t, 0);
    if (k % 4u == 1u) e.send_remove(t, 1);
    if (k % 8u == 2u) e.send_insert(t, 1);
    if (k % 61u == 17u) e.send_despawn(t);
    if (k % 37u == 0u && e.slot % 11ull == 5ull) e.despawn();          // a sender that despawns itself in the same call still sends
}
"""
# the same world registered WITHOUT remote bindings (the launch-count comparison): the striker only reads its link
STRIKER_NONE_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u32 k = (ggrs_u32)e.slot + (ggrs_u32)f.frame;
    if (k % 37u == 0u && e.slot % 11ull == 5ull) e.despawn();
}
"""
# the comparison world of scripts/bench_remote_commands.py: Stun ALWAYS present (ticks 0 = "absent"), the striker writes it through effects -- MAX_U of the
# default ticks into Stun.ticks, OR of the default seed into Stun.seed; no Shield, no despawn
STRIKER_FX_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u64 t = e.u64(0);
    const ggrs_u32 k = (ggrs_u32)e.slot + (ggrs_u32)f.frame;
    if (k % 3u == 0u) { e.send_u32(t, 0, 5u); e.send_u32(t, 1, 77u); }
}
"""
COUNTDOWN_OWN_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    e.u32(0) = e.u32(0) + (ggrs_u32)f.input[0];
    if (e.u32(1) >= 1u) e.u32(1) -= 1u;
}
"""
# the remote-stun world of the bench: only the insert of Stun
STRIKER_STUN_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u64 t = e.u64(0);
    const ggrs_u32 k = (ggrs_u32)e.slot + (ggrs_u32)f.frame;
    if (k % 3u == 0u) e.send_insert(t, 0);
}
"""
# binding 0 = Target, 1 = Seen; peer binding 0 = Stun.ticks
WATCH_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) {
    const GgrsPeer p = e.peer(e.u64(0));
    e.u32(1) = e.u32(1) + (p.ok() ? 1u + p.u32(0) : 100u);
}
"""
CHILD_SRC = r"""
struct Child { ggrs_u32 hp, pad; ggrs_u64 target; };
__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64, const GgrsFrame&, const unsigned char* payload) {      // commands.spawn((Hp, Target, Rollback))
    const Child* c = reinterpret_cast<const Child*>(payload);
    e.u32(0) = c->hp; e.u64(1) = c->target;
}
"""
CHILD_STRIDE = 16
CHILD_DT = np.dtype([("hp", "<u4"), ("pad", "<u4"), ("target", "<u8")])


class Stats:
    """What the oracle's strikers sent and what became of it, over a session (every simulated frame counts, re-simulated ones too)."""

    def __init__(self):
        self.sent = self.landed = 0
        self.ins_absent = self.ins_present = self.removes = self.despawns = 0       # landed, by what they did
        self.despawn_and_insert = self.insert_and_remove = 0                        # conflicts on one live target
        self.out_of_range = self.dead_target = self.spawned_this_frame = 0          # dropped
        self.dead_sender = 0                                                        # commands of senders that despawned themselves in the same call
        self.frames = 0

    def floors(self):
        return {"ins_absent": self.ins_absent, "ins_present": self.ins_present, "removes": self.removes, "despawns": self.despawns,
                "despawn_and_insert": self.despawn_and_insert, "insert_and_remove": self.insert_and_remove, "out_of_range": self.out_of_range,
                "dead_target": self.dead_target, "spawned_this_frame": self.spawned_this_frame, "dead_sender": self.dead_sender}


class _Cmds:
    """The commands of the striker's current pass, per target slot below n0 (the len at the start of the frame): counts of senders."""

    def __init__(self):
        self.n0 = 0
        self.ins_stun = self.rem_sh = self.ins_sh = self.desp = self.any = None
        self.pending = None                                                         # (frame, n0, [out-of-range targets]) of the previous pass


def _countdown_fn(o, S):
    c = _Pass()

    def countdown(words, slot, f):
        if c.begin(slot, f.frame):
            n = o.len
            c.has = o.present_mask(S, n).tolist(); c.ticks = o.download_word(S, 0, 0, n).tolist()
        hp = (words[0] + f.input(0)[0]) & M32
        if c.has[slot]:
            if c.ticks[slot] <= 1: o.remove_component(S, slot)
            else: o.upload_word(S, 0, slot, np.array([c.ticks[slot] - 1], dtype=U32))
        return [hp], 0
    return countdown


def build_hit(w, *, with_spawn=False, watcher=False, remote=True, st=None):
    """Registers the hit world on `w` (a library world or the oracle); returns the component ids (Hp, Target, Stun, Shield[, Seen]).  st: the oracle's Stats.
    remote=False (library worlds): the same systems with a striker that commands nothing -- the launch-count comparison."""
    H = w.register_component("Hp", 4, 1)
    T = w.register_component("Target", 8, 1)
    S = w.register_component("Stun", 4, 2)
    SH = w.register_component("Shield", 8, 1)
    ids = [H, T, S, SH]
    w.set_component_default(S, np.array(STUN_DEFAULT, dtype=U32))
    w.set_component_default(SH, np.array([SHIELD_DEFAULT], dtype=U64))
    for c, words in ((H, [0]), (T, [0]), (S, [0, 1]), (SH, [0])): w.checksum_component(c, words)
    if watcher:
        N = w.register_component("Seen", 4, 1); w.checksum_component(N, [0]); ids.append(N)
    if isinstance(w, OracleWorld):
        st = st if st is not None else Stats()
        cm_, ps, pw = _Cmds(), _Pass(), _Pass()

        def watch(words, slot, f):
            if pw.begin(slot, f.frame):
                n = w.len
                pw.vis = (w.alive_mask(n) & w.present_mask(S, n)).tolist()      # the peer view at the start of the frame (the watcher is the first system)
                pw.ticks, pw.n = w.download_word(S, 0, 0, n).tolist(), n
            t = words[0]
            ok = t < pw.n and pw.vis[t]
            return [t, (words[1] + (1 + pw.ticks[t] if ok else 100)) & M32], 0

        def strike(words, slot, f):
            if ps.begin(slot, f.frame):
                n = w.len
                tg = w.download_word(T, 0, 0, n).astype(U64, copy=False)
                alive = w.alive_mask(n)
                on = alive & w.present_mask(T, n)                               # the entities the striker runs for
                i = np.arange(n, dtype=np.int64)
                k = (i + f.frame).astype(U32)
                c_is, c_rs, c_ish, c_d = on & (k % U32(3) == 0), on & (k % U32(4) == 1), on & (k % U32(8) == 2), on & (k % U32(61) == 17)
                kill = on & (k % U32(37) == 0) & (i % 11 == 5)
                in_range = tg < U64(n)
                ti = np.where(in_range, tg, 0).astype(np.int64)
                def per_target(c):
                    a = np.zeros(n, dtype=np.int64); np.add.at(a, ti[c & in_range], 1); return a
                a_is, a_rs, a_ish, a_d = per_target(c_is), per_target(c_rs), per_target(c_ish), per_target(c_d)
                n_cmd = c_is.astype(np.int64) + c_rs + c_ish + c_d                 # commands per sender
                # the previous pass's out-of-range targets that exist now were spawned in its frame: dropped as "spawned this frame"
                if cm_.pending is not None and cm_.pending[0] + 1 == f.frame and n > cm_.pending[1]:
                    st.spawned_this_frame += int(((cm_.pending[2] >= cm_.pending[1]) & (cm_.pending[2] < n)).sum())
                oor = np.repeat(tg[~in_range & on], n_cmd[~in_range & on])
                cm_.pending = (f.frame, n, oor.astype(np.int64))
                cm_.n0 = n
                cm_.ins_stun, cm_.rem_sh, cm_.ins_sh, cm_.desp = a_is.tolist(), a_rs.tolist(), a_ish.tolist(), a_d.tolist()
                cm_.any = ((a_is + a_rs + a_ish + a_d) > 0).tolist()
                cm_.kill = kill.tolist()
                st.frames += 1
                st.sent += int(n_cmd.sum())
                st.out_of_range += int(n_cmd[~in_range].sum())
                st.dead_sender += int(n_cmd[kill].sum())
                # a target that is dead when the pass begins stays dead: its commands are dropped (a lower bound: targets that die in this frame drop theirs too)
                st.dead_target += int((a_is + a_rs + a_ish + a_d)[~alive].sum())
            return list(words), int(cm_.kill[slot])

        def apply(words, slot, f):
            # (runs for live entities that have Target: alive once the frame's own despawns are in)
            if slot >= cm_.n0 or not cm_.any[slot]: return list(words), 0
            n_is, n_rs, n_ish, n_d = cm_.ins_stun[slot], cm_.rem_sh[slot], cm_.ins_sh[slot], cm_.desp[slot]
            st.landed += n_is + n_rs + n_ish + n_d
            if n_rs and n_ish: st.insert_and_remove += 1                         # (counted on every live target that got both, also one a despawn then takes)
            if n_d:                                                               # despawn wins over everything
                st.despawns += 1
                if n_is or n_ish: st.despawn_and_insert += 1
                return list(words), 1
            if n_is:
                if w.present_mask(S, slot + 1)[slot]: st.ins_present += 1
                else: st.ins_absent += 1
                w.insert_component(S, slot, np.array(STUN_DEFAULT, dtype=U32))
            if n_rs:                                                              # remove wins over insert
                if w.present_mask(SH, slot + 1)[slot]: w.remove_component(SH, slot); st.removes += 1
            elif n_ish:
                if w.present_mask(SH, slot + 1)[slot]: st.ins_present += 1
                else: st.ins_absent += 1
                w.insert_component(SH, slot, np.array([SHIELD_DEFAULT], dtype=U64))
            return list(words), 0

        def child(words, slot, k, f, payload):
            rec = np.frombuffer(bytes(payload[:CHILD_STRIDE]), dtype=CHILD_DT)[0]
            return [int(rec["hp"]), int(rec["target"])]
        if watcher: w.add_custom_system(watch, [(T, 0), (ids[4], 0)])
        w.add_custom_system(_countdown_fn(w, S), [(H, 0)])
        w.add_custom_system(strike, [(T, 0)])
        w.add_custom_system(apply, [(T, 0)])
        if with_spawn: w.add_spawn_system(child, bundle=(H, T), bindings=[(H, 0), (T, 0)], payload_stride=CHILD_STRIDE)
    else:
        if watcher: w.add_custom_system(WATCH_SRC, [(T, 0), (ids[4], 0)], name="watcher", peers=[(S, 0)])
        w.add_custom_system(COUNTDOWN_SRC, [(H, 0)], name="countdown", commands=[(S, bg.CMD_REMOVE)])
        if remote:
            w.add_custom_system(STRIKER_SRC, [(T, 0)], name="striker",
                                remote=[(S, bg.REMOTE_INSERT), (SH, bg.REMOTE_INSERT | bg.REMOTE_REMOVE), (bg.REMOTE_ENTITY, bg.REMOTE_DESPAWN)])
        else: w.add_custom_system(STRIKER_NONE_SRC, [(T, 0)], name="striker")
        if with_spawn: w.add_spawn_system(CHILD_SRC, bundle=(H, T), bindings=[(H, 0), (T, 0)], payload_stride=CHILD_STRIDE, name="child")
    return tuple(ids)


def spawn_hit(w, ids, n, *, links=None):
    """n entities with Hp and Target (and Seen); every fourth also has Shield (charges above 2^32).  Links: strike_links -- (i * 389 + 17) % n, every 13th at slot 0
    (contention on one inbox word), every 10th out of range (n + 5: in the spawn variant that slot appears mid-session)."""
    H, T, S, SH = ids[:4]
    i = np.arange(n)
    bundle = {H: [((i * 37 + 11) % 101).astype(U32)], T: [strike_links(n) if links is None else links]}
    if len(ids) > 4: bundle[ids[4]] = [np.zeros(n, dtype=U32)]
    w.spawn(n, bundle)
    for s in range(0, n, 4): w.insert_component(SH, s, np.array([0x300000000 + (s % 23)], dtype=U64))


def children(frame, n0):
    """The host side of the spawn system, a pure function of the frame: in every fourth frame five children that link to existing slots."""
    if frame % 4 != 1: return 0, None
    r = np.random.default_rng([6, frame])
    rec = np.zeros(5, dtype=CHILD_DT)
    rec["hp"] = r.integers(0, 30, 5); rec["target"] = r.integers(0, n0, 5)
    return 5, rec


def spawn_patch(n0):
    def patch(frame, r):
        cnt, rec = children(frame, n0)
        if cnt: r.spawn_count, r.spawn_payload = cnt, rec
    return patch


def p2p_lists():
    """P2P-shaped lists: plain ticks, then a rollback of 3, more ticks, then a rollback of 1 -- [Load(F - k), (Advance, Save) x (k + 1)]."""
    lists = [[bg.SaveGameState(0), bg.AdvanceFrame((1,)), bg.SaveGameState(1)]]
    F = 1
    for k in (0, 0, 0, 0, 3, 0, 0, 1, 0, 0):
        reqs = [bg.LoadGameState(F - k)]
        for i in range(k + 1): reqs += [bg.AdvanceFrame(((F - k + i) % 3,)), bg.SaveGameState(F - k + i + 1)]
        lists.append(reqs); F += 1
    return lists
