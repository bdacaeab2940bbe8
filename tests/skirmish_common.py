"""The "skirmish" world: ONE user-written system that carries every binding kind at once -- peer reads, effects, own-entity commands (in the system ahead of it),
remote commands, resource reads, reducers and float sums -- built twice: on a library world from HIP C++ source, and on the CPU oracle (oracle.binding.OracleWorld,
unchanged) from Python callbacks with sums_common.SumModel beside it.  `kinds` is a frozenset over KINDS; the striker's source and binding lists are assembled from
fragments by kind, so every subset gives a legal world with the same components, resources and spawn data.

    Pos {x, y} 2 x f32 (sums_common.flock_xy: the ORDER of a float sum shows)     Target u64 (peer_effects_common.strike_links)     Armor u32 (written by no system: the peer column)
    Hp u32, Score u64 (the effect columns)      Stun {ticks, seed} 2 x u32, absent at spawn, default {5, 77}      Shield u64, default 0xABCD00000007, on every fourth entity
    Fuse u32 (GGRS_SYS_SAT_SUB_DESPAWN: entities die mid-session)
    resources  Clock{u32}   Centre{f32 sx, f32 sy}   Energy{f64, never reset}   Census{u32 alive: ADD, u32 worst: MAX_U}          everything is checksummed

    tick       (kind res) resource system: Clock += 1 + input; sx = sy = 0; alive = 0
    countdown  own binding Hp: hp += input; (kind commands) command binding Stun with CMD_REMOVE: a stunned entity counts down and loses Stun at 1
    striker    own bindings Target, Pos.x, Pos.y.  k = slot + frame (+ Clock, kind res: a frame re-simulated with another input sends other commands);
               dmg = 1 + k % 5 + (kind peer: Armor of the target & 3, or 7 where the peer is not visible; else: the bits of its own x & 3)
               effects   ADD of 0 - dmg (wrapping) to the target's Hp, ADD of 2^32 + dmg to its Score
               remote    insert Stun / remove Shield / insert Shield / despawn on the hit world's conditions of k
               reduces   +1 into alive, MAX_U of dmg into worst
               sums      x into sx, y into sy, (double)x * x into Energy
               always    a few strikers despawn themselves in the same call (and still send, reduce and sum)
    fuse       GGRS_SYS_SAT_SUB_DESPAWN on Fuse
    child      (with_spawn) a host-decided spawn system, as in the hit world

THE ORDER.  The fuse countdown is registered BEHIND the striker, not first: a system with peer bindings is registered before every other system that can despawn
(host_seal.hpp peers_validate; the peer view is the world at the start of the frame), and the countdown binds Hp and commands Stun, so it is registered ahead of the
system that sends to Hp and remotely commands Stun.  tick, countdown, striker, fuse is the one order every subset seals in; test_skirmish_text.py pins the refusal
of the other one.  An entity whose fuse runs out dies in the frame AFTER its striker call: it is one more "doomed" sender.

On the oracle the striker commands nothing.  At the start of its pass it computes the whole pass vectorised in numpy from the oracle's own columns (kept only for slots
below the len at the start of the frame) and feeds the model's sum / reduce per slot for the entities it runs for.  The callbacks registered LAST apply, in the
library's order: the remote apply (despawn wins, remove wins over insert), then one effect apply per effect column -- which the oracle runs only for entities alive
once the remote despawns are in.  reduces_common.run_model calls model.end() behind the frame.
(A helper module, no tests of its own.)"""
import functools

import numpy as np

import bevy_ggrs_amd as bg
import common as cm
import reduces_common as rd
import remote_commands_common as rc
import sums_common as sc
from oracle.binding import FLAT, OracleWorld
from peer_effects_common import _Pass, strike_links, synctest_lists
from remote_commands_common import SHIELD_DEFAULT, STUN_DEFAULT

U32, U64 = np.uint32, np.uint64
F32, F64 = np.float32, np.float64
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
DEPTH = 8
KINDS = ("peer", "effects", "commands", "remote", "res", "reduces", "sums")
ALL = frozenset(KINDS)
NONE = frozenset()


def _s(*names): return frozenset(names)


# A covering list: for every pair of kinds all four on / off combinations occur (test_skirmish_text.py asserts it), plus the subsets at which the generator and the
# host policy branch: remote without effects (rx_len is a field of its own) and with them (the remote path reads fx_len), sums without reduces and reduces without
# sums (k_apply_sums / k_apply_reduces alone), remote + sums with neither effects nor reduces (value tags: off for remote, on for sums).
GPU_SUBSETS = (
    ALL,
    _s("remote"),                                                   # {remote} - effects
    _s("remote", "effects"),
    _s("sums"),                                                     # {sums} - reduces
    _s("reduces"),                                                  # {reduces} - sums
    _s("remote", "sums"),                                           # neither effects nor reduces
    _s("peer", "effects", "res"),
    _s("peer", "commands", "reduces", "sums"),
    _s("effects", "commands", "res", "reduces"),
    _s("peer", "commands", "remote", "res"),
    _s("effects", "commands", "sums"),
    NONE,
)


def subset_id(kinds):
    return "+".join(k for k in KINDS if k in kinds) or "none"


# ---- the library side: sources assembled from fragments ---------------------------------------------------------------------------------------------------------
TICK_SRC = r"""
__device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame& f) {
    r.u32(0) += 1u + (ggrs_u32)f.input[0];
    r.f32(1) = 0.f; r.f32(2) = 0.f; r.u32(3) = 0u;
}
"""
COUNTDOWN_PLAIN_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) { e.u32(0) = e.u32(0) + (ggrs_u32)f.input[0]; }"
CHILD_SRC = r"""
struct Child { float x, y; ggrs_u32 hp, armor; ggrs_u64 target; };
__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64, const GgrsFrame&, const unsigned char* payload) {      // commands.spawn((Pos, Target, Armor, Hp, Score, Rollback))
    const Child* c = reinterpret_cast<const Child*>(payload);
    e.f32(0) = c->x; e.f32(1) = c->y; e.u64(2) = c->target; e.u32(3) = c->armor; e.u32(4) = c->hp;
}
"""
CHILD_STRIDE = 24
CHILD_DT = np.dtype([("x", "<f4"), ("y", "<f4"), ("hp", "<u4"), ("armor", "<u4"), ("target", "<u8")])


def striker_source(kinds):
    """own bindings 0 = Target, 1 = Pos.x, 2 = Pos.y; peer binding 0 = Armor; effect bindings 0 = Hp, 1 = Score; remote bindings 0 = Stun (INSERT), 1 = Shield
    (INSERT | REMOVE), 2 = the entity (DESPAWN); resource binding 0 = Clock; reduce bindings 0 = alive, 1 = worst; sum bindings 0 = sx, 1 = sy, 2 = Energy."""
    L = ["__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {",
         "    const ggrs_u64 t = e.u64(0);",
         "    const ggrs_u32 k = (ggrs_u32)e.slot + (ggrs_u32)f.frame" + (" + e.res_u32(0);" if "res" in kinds else ";")]
    if "peer" in kinds: L += ["    const GgrsPeer p = e.peer(t);", "    const ggrs_u32 dmg = 1u + k % 5u + (p.ok() ? (p.u32(0) & 3u) : 7u);"]
    else: L += ["    const ggrs_u32 dmg = 1u + k % 5u + (__float_as_uint(e.f32(1)) & 3u);"]
    if "effects" in kinds: L += ["    e.send_u32(t, 0, 0u - dmg);", "    e.send_u64(t, 1, 0x100000000ull + dmg);"]
    if "remote" in kinds:
        L += ["    if (k % 3u == 0u) e.send_insert(t, 0);", "    if (k % 4u == 1u) e.send_remove(t, 1);", "    if (k % 8u == 2u) e.send_insert(t, 1);",
              "    if (k % 61u == 17u) e.send_despawn(t);"]
    if "reduces" in kinds: L += ["    e.reduce_u32(0, 1u);", "    e.reduce_u32(1, dmg);"]
    if "sums" in kinds: L += ["    e.sum_f32(0, e.f32(1));", "    e.sum_f32(1, e.f32(2));", "    e.sum_f64(2, (double)e.f32(1) * (double)e.f32(1));"]
    L += ["    if ((t ^ dmg) == 0xFFFFFFFFFFFFFFFFull) e.u64(0) = t;",              # (no kind uses t or dmg in the empty subset: no unused-variable warning)
          "    if (k % 37u == 0u && e.slot % 11ull == 5ull) e.despawn();          // a sender that despawns itself in the same call still sends, reduces and sums",
          "}"]
    return "\n".join(L) + "\n"


def striker_bindings(kinds, ids, res):
    """The keyword arguments of World.add_custom_system for the striker of `kinds`."""
    P, T, A, H, Sc, S, SH, Fz = ids
    Ck, Ce, En, Cn = res
    kw = {}
    if "peer" in kinds: kw["peers"] = [(A, 0)]
    if "effects" in kinds: kw["effects"] = [(H, 0, bg.EFFECT_ADD), (Sc, 0, bg.EFFECT_ADD)]
    if "remote" in kinds: kw["remote"] = [(S, bg.REMOTE_INSERT), (SH, bg.REMOTE_INSERT | bg.REMOTE_REMOVE), (bg.REMOTE_ENTITY, bg.REMOTE_DESPAWN)]
    if "res" in kinds: kw["resources"] = [(Ck, 0)]
    if "reduces" in kinds: kw["reduces"] = [(Cn, 0, bg.EFFECT_ADD), (Cn, 1, bg.EFFECT_MAX_U)]
    if "sums" in kinds: kw["sums"] = [(Ce, 0), (Ce, 1), (En, 0)]
    return kw


# ---- the model beside the oracle --------------------------------------------------------------------------------------------------------------------------------
ENERGY_INIT = sc.f64_bits(0.5)
CLOCK, CENTRE, ENERGY, CENSUS = 0, 1, 2, 3


def skirmish_layout(kinds):
    s = sc.SUM if "sums" in kinds else None
    return [("Clock", 4, [(0, None)]), ("Centre", 4, [(0, s), (0, s)]), ("Energy", 8, [(ENERGY_INIT, s)]),
            ("Census", 4, [(0, bg.EFFECT_ADD if "reduces" in kinds else None), (0, bg.EFFECT_MAX_U if "reduces" in kinds else None)])]


def skirmish_model(kinds, n_slots):
    def tick(cur, inp0):
        cur[CLOCK][0] = (cur[CLOCK][0] + 1 + (inp0 & 0xFF)) & M32
        cur[CENTRE][0] = 0; cur[CENTRE][1] = 0; cur[CENSUS][0] = 0
    return sc.SumModel(skirmish_layout(kinds), n_slots, tick if "res" in kinds else None)


class Stats:
    """What the oracle's strikers sent and what became of it, over a session (every simulated frame counts, re-simulated ones too), and the cross-feature events
    no single-feature suite can produce."""

    def __init__(self):
        self.fx_sent = self.fx_landed = self.rx_sent = self.rx_landed = 0
        # effect sends dropped because the target was remotely despawned in the same frame.  This pins the ORACLE's bookkeeping (the frames in which the rule
        # decides exist): on the device a dropped and an applied effect on a slot that is dead by then leave the same checksummed state -- only the alive and
        # presence bits the effect apply reads are observable, not whether it wrote the dead slot's column.
        self.effect_on_remotely_despawned = 0
        self.reduced_by_doomed = 0                     # reductions from an entity that is remotely despawned, or despawns itself, in the same frame: they count
        self.summed_by_doomed = 0                      # ... and sums
        self.own_remove_and_remote_insert = 0          # Stun removed by the entity's own countdown AND remotely inserted in one frame: present, with the default
        self.spawned_this_frame_dropped = 0            # commands and effects to an entity spawned in this frame
        self.frames = 0

    def cross(self, with_spawn=False):
        names = ("effect_on_remotely_despawned", "reduced_by_doomed", "summed_by_doomed", "own_remove_and_remote_insert") + (("spawned_this_frame_dropped",) if with_spawn else ())
        return {k: getattr(self, k) for k in names}


class _Sent:
    """The striker's current pass, per slot below n0 (the len at the start of the frame)."""

    def __init__(self):
        self.n0, self.frame = 0, None
        self.pending = None                             # (frame, n0, out-of-range targets, one per command or effect sent there) of the previous pass


def build_skirmish(w, kinds=ALL, *, with_spawn=False, bare_striker=False, fuse_first=False, model=None, st=None, host_apply=False):
    """Registers the skirmish world on `w` (a library world, or the oracle with its model); returns the component ids (Pos, Target, Armor, Hp, Score, Stun, Shield,
    Fuse).  bare_striker (a library world): the same world whose striker binds nothing but its own words -- the launch-count comparison.  fuse_first (a library world):
    the fuse countdown registered first -- the order the peer rule refuses.  host_apply (the oracle): the apply callbacks are NOT registered as systems -- a system
    runs only for entities that have its bound component, so an entity without Target would take no remote command --; the driver calls w.land() behind every
    AdvanceFrame instead, which runs the same callbacks by host calls for every entity alive at the end of the frame (tests/fuzz_user_worlds.py)."""
    kinds = frozenset(kinds)
    assert kinds <= ALL, kinds
    P = w.register_component("Pos", 4, 2); T = w.register_component("Target", 8, 1); A = w.register_component("Armor", 4, 1)
    H = w.register_component("Hp", 4, 1); Sc = w.register_component("Score", 8, 1)
    S = w.register_component("Stun", 4, 2); SH = w.register_component("Shield", 8, 1); Fz = w.register_component("Fuse", 4, 1)
    ids = (P, T, A, H, Sc, S, SH, Fz)
    w.set_component_default(S, np.array(STUN_DEFAULT, dtype=U32))
    w.set_component_default(SH, np.array([SHIELD_DEFAULT], dtype=U64))
    for c in ids: w.checksum_component(c, list(range(2 if c in (P, S) else 1)))
    own = [(T, 0), (P, 0), (P, 1)]
    child_binds = [(P, 0), (P, 1), (T, 0), (A, 0), (H, 0)]
    fuse = lambda: w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(Fz,), word=(0,), iparam=(1, bg.DESPAWN_IMMEDIATE))      # noqa: E731
    if not isinstance(w, OracleWorld):
        res = sc.register_model_resources(w, skirmish_model(kinds, 1))
        Ck, Ce, En, Cn = res
        if fuse_first: fuse()
        if "res" in kinds: w.add_resource_system(TICK_SRC, [(Ck, 0), (Ce, 0), (Ce, 1), (Cn, 0)], name="tick")
        if "commands" in kinds: w.add_custom_system(rc.COUNTDOWN_SRC, [(H, 0)], name="countdown", commands=[(S, bg.CMD_REMOVE)])
        else: w.add_custom_system(COUNTDOWN_PLAIN_SRC, [(H, 0)], name="countdown")
        sk = NONE if bare_striker else kinds
        w.add_custom_system(striker_source(sk), own, name="striker", **striker_bindings(sk, ids, res))
        if not fuse_first: fuse()
        if with_spawn: w.add_spawn_system(CHILD_SRC, bundle=(P, T, A, H, Sc), bindings=child_binds, payload_stride=CHILD_STRIDE, name="child")
        return ids
    st = st if st is not None else Stats()
    sn, pc, ps = _Sent(), _Pass(), _Pass()
    pc.removed, pc.frame_ = set(), None

    def countdown(words, slot, f):
        if pc.begin(slot, f.frame):
            n = w.len
            pc.removed, pc.frame_ = set(), f.frame
            if "commands" in kinds: pc.has = w.present_mask(S, n).tolist(); pc.ticks = w.download_word(S, 0, 0, n).tolist()
        hp = (words[0] + f.input(0)[0]) & M32
        if "commands" in kinds and pc.has[slot]:
            if pc.ticks[slot] <= 1: w.remove_component(S, slot); pc.removed.add(slot)
            else: w.upload_word(S, 0, slot, np.array([pc.ticks[slot] - 1], dtype=U32))
        return [hp], 0

    def begin_pass(f):
        n = w.len
        tg = w.download_word(T, 0, 0, n).astype(U64, copy=False)
        px = w.download_word(P, 0, 0, n).astype(U32, copy=False); py = w.download_word(P, 1, 0, n).astype(U32, copy=False)
        alive = w.alive_mask(n)
        on = alive & w.present_mask(T, n) & w.present_mask(P, n)                # the entities the striker runs for
        i = np.arange(n, dtype=np.int64)
        clock = model.cur[CLOCK][0] if "res" in kinds else 0                     # (tick is registered ahead of the striker: the value AFTER it ran)
        k = ((i + f.frame + clock) & M32).astype(U32)
        in_range = tg < U64(n)
        ti = np.where(in_range, tg, 0).astype(np.int64)
        if "peer" in kinds:
            vis = alive & w.present_mask(A, n)                                   # the peer view: no system ahead of the striker despawns, nobody writes Armor
            armor = w.download_word(A, 0, 0, n).astype(U32, copy=False)
            extra = np.where(in_range & vis[ti], armor[ti] & U32(3), U32(7)).astype(U32)
        else: extra = px & U32(3)
        dmg = (U32(1) + k % U32(5) + extra).astype(U32)
        kill = on & (k % U32(37) == 0) & (i % 11 == 5)
        sn.n0, sn.frame, sn.on, sn.kill, sn.dmg = n, f.frame, on.tolist(), kill.tolist(), dmg.tolist()
        x, y = px.view(F32), py.view(F32)
        sn.x, sn.y, sn.xx = x, y, x.astype(F64) * x.astype(F64)
        send = on & in_range
        t = ti[send]
        # effects: the combined value and the number of senders per target
        hp = np.zeros(n, dtype=U32); score = np.zeros(n, dtype=U64); cnt = np.zeros(n, dtype=np.int64)
        if "effects" in kinds:
            np.add.at(hp, t, (U32(0) - dmg[send]).astype(U32)); np.add.at(score, t, U64(0x100000000) + dmg[send].astype(U64)); np.add.at(cnt, t, 1)
            st.fx_sent += 2 * int(on.sum())
        sn.fx_val, sn.fx_cnt = (hp.tolist(), score.tolist()), cnt.tolist()
        # remote commands: the number of senders per target and command
        zero = np.zeros(n, dtype=bool)
        conds = (on & (k % U32(3) == 0), on & (k % U32(4) == 1), on & (k % U32(8) == 2), on & (k % U32(61) == 17)) if "remote" in kinds else (zero,) * 4

        def per_target(c):
            a = np.zeros(n, dtype=np.int64); np.add.at(a, ti[c & in_range], 1); return a
        a_is, a_rs, a_ish, a_d = (per_target(c) for c in conds)
        n_cmd = sum(c.astype(np.int64) for c in conds)
        sn.ins_stun, sn.rem_sh, sn.ins_sh, sn.desp = a_is.tolist(), a_rs.tolist(), a_ish.tolist(), a_d.tolist()
        sn.any = ((a_is + a_rs + a_ish + a_d) > 0).tolist()
        st.rx_sent += int(n_cmd.sum())
        # what the previous pass sent out of range to slots that exist now was sent to entities spawned in ITS frame: dropped
        per_sender = n_cmd + (2 if "effects" in kinds else 0)
        if sn.pending is not None and sn.pending[0] + 1 == f.frame and n > sn.pending[1]:
            st.spawned_this_frame_dropped += int(((sn.pending[2] >= sn.pending[1]) & (sn.pending[2] < n)).sum())
        sn.pending = (f.frame, n, np.repeat(tg[~in_range & on], per_sender[~in_range & on]).astype(np.int64))
        # a striker that despawns itself in this call is doomed; the remotely despawned ones are counted where the despawn lands
        n_kill = int(kill.sum())
        if "reduces" in kinds: st.reduced_by_doomed += 2 * n_kill
        if "sums" in kinds: st.summed_by_doomed += 3 * n_kill
        st.frames += 1

    def strike(words, slot, f):
        if ps.begin(slot, f.frame): begin_pass(f)
        if "reduces" in kinds: model.reduce(CENSUS, 0, 1); model.reduce(CENSUS, 1, sn.dmg[slot])
        if "sums" in kinds: model.sum(CENTRE, 0, slot, sn.x[slot]); model.sum(CENTRE, 1, slot, sn.y[slot]); model.sum(ENERGY, 0, slot, sn.xx[slot])
        return list(words), int(sn.kill[slot])

    def apply_remote(words, slot, f):
        # (runs for live entities that have Target: alive once the frame's own despawns -- the strikers' and the fuse's -- are in)
        if sn.frame != f.frame or slot >= sn.n0 or not sn.any[slot]: return list(words), 0
        n_is, n_rs, n_ish, n_d = sn.ins_stun[slot], sn.rem_sh[slot], sn.ins_sh[slot], sn.desp[slot]
        st.rx_landed += n_is + n_rs + n_ish + n_d
        if n_d:                                                               # despawn wins over everything; the effect applies behind this one skip the entity
            st.effect_on_remotely_despawned += 2 * sn.fx_cnt[slot]
            if sn.on[slot]:
                if "reduces" in kinds: st.reduced_by_doomed += 2
                if "sums" in kinds: st.summed_by_doomed += 3
            return list(words), 1
        if n_is:
            if pc.frame_ == f.frame and slot in pc.removed: st.own_remove_and_remote_insert += 1
            w.insert_component(S, slot, np.array(STUN_DEFAULT, dtype=U32))
        if n_rs:                                                              # remove wins over insert
            if w.present_mask(SH, slot + 1)[slot]: w.remove_component(SH, slot)
        elif n_ish: w.insert_component(SH, slot, np.array([SHIELD_DEFAULT], dtype=U64))
        return list(words), 0

    def make_apply(j, mask):
        def apply(words, slot, f):
            if sn.frame != f.frame or slot >= sn.n0 or not sn.fx_cnt[slot]: return list(words), 0
            st.fx_landed += sn.fx_cnt[slot]
            return [(words[0] + sn.fx_val[j][slot]) & mask], 0
        return apply

    def begin_frame():
        """For a driver that may advance one frame twice in a row, or advance a frame in which the striker runs for nobody (tests/fuzz_user_worlds.py calls it
        before every AdvanceFrame): every pass starts anew, and what the previous frame sent is forgotten -- nothing is applied unless the striker runs again."""
        pc.reset(); ps.reset()
        pc.removed, pc.frame_ = set(), None
        sn.n0, sn.frame = 0, None
    w.begin_frame = begin_frame

    def on_load():
        """Behind a LoadGameState: the previous pass belongs to another timeline, so what it sent out of range is not held against the next pass's len."""
        sn.pending = None
    w.on_load = on_load

    def land():
        """The applies by host calls, in the library's order: the remote apply for every entity alive at the end of the frame (whatever components it has), then one
        effect apply per column for the entities alive after that which have the column."""
        if sn.frame is None: return                                             # the striker ran for nobody: nothing was sent
        class F: frame = sn.frame      # noqa: E701
        n = min(sn.n0, w.len)
        if "remote" in kinds:
            alive = w.alive_mask(n)
            for slot in range(n):
                if alive[slot] and sn.any[slot] and apply_remote([], slot, F)[1]: w.despawn(slot)
        if "effects" in kinds:
            alive = w.alive_mask(n)
            for j, (c, mask, dt) in enumerate(((H, M32, U32), (Sc, M64, U64))):
                on = alive & w.present_mask(c, n)
                col = w.download_word(c, 0, 0, n)
                fn = make_apply(j, mask)
                for slot in np.nonzero(on)[0].tolist():
                    if sn.fx_cnt[slot]: w.upload_word(c, 0, slot, np.array([fn([int(col[slot])], slot, F)[0][0]], dtype=dt))
    w.land = land

    def child(words, slot, k, f, payload):
        rec = np.frombuffer(bytes(payload[:CHILD_STRIDE]), dtype=CHILD_DT)[0]
        return [int(np.array([rec["x"]], dtype=F32).view(U32)[0]), int(np.array([rec["y"]], dtype=F32).view(U32)[0]), int(rec["target"]), int(rec["armor"]), int(rec["hp"])]
    w.add_custom_system(countdown, [(H, 0)])
    w.add_custom_system(strike, own)
    fuse()
    if "remote" in kinds and not host_apply: w.add_custom_system(apply_remote, [(T, 0)])
    if "effects" in kinds and not host_apply:
        w.add_custom_system(make_apply(0, M32), [(H, 0)]); w.add_custom_system(make_apply(1, M64), [(Sc, 0)])
    if with_spawn: w.add_spawn_system(child, bundle=(P, T, A, H, Sc), bindings=child_binds, payload_stride=CHILD_STRIDE)
    return ids


# Where the positions start in sums_common.order_values.  The squares of 24-bit floats are exact in a double and their sum rounds rarely, so for most starting points
# some order of adding them gives the tree's bits; from 13 on the tree total of x, of y AND of x * x differs from the slot-order, the reverse-order and the
# sequential-per-64-then-sequential total at 257 and at 1025 entities (test_skirmish_text.py asserts it; from 0 the per-64 order gives the tree's Energy at 1025).
XY_FIRST = 13


def spawn_skirmish(w, ids, n, *, links=None, fuse=None):
    """n entities with everything but Stun; every fourth also has Shield (charges above 2^32).  Links: strike_links -- (i * 389 + 17) % n, every 13th at slot 0, every
    10th out of range (n + 5: in the spawn variant that slot appears mid-session).  A fifth starts with Hp below the first damage: the ADD wraps.
    fuse: the n fuses, where 4 .. 48 frames (9 for a lone entity) are too short for the session."""
    P, T, A, H, Sc, S, SH, Fz = ids
    i = np.arange(n)
    x, y = sc.flock_xy(XY_FIRST, n)
    if fuse is None: fuse = (4 + (i * 7) % 45).astype(U32) if n > 1 else np.array([9], dtype=U32)
    fuse = np.ascontiguousarray(fuse, dtype=U32)
    w.spawn(n, {P: [x.view(U32), y.view(U32)], T: [strike_links(n) if links is None else links], A: [((i * 5 + 2) % 13).astype(U32)],
                H: [np.where(i % 5 == 1, i % 3, 300 + (i * 37 + 11) % 101).astype(U32)], Sc: [(i.astype(U64) << U64(33)) | U64(7)], Fz: [fuse]})
    for s in range(0, n, 4): w.insert_component(SH, s, np.array([0x300000000 + (s % 23)], dtype=U64))


def children(frame, n0, period=4):
    """The host side of the spawn system, a pure function of the frame: in every fourth (`period`-th) frame five children that link to existing slots."""
    if frame % period != 1 % period: return 0, None
    r = np.random.default_rng([6, frame])
    rec = np.zeros(5, dtype=CHILD_DT)
    xy = sc.order_values(10, 5000 + 10 * frame)
    rec["x"], rec["y"] = xy[:5], xy[5:]
    rec["hp"] = r.integers(0, 30, 5); rec["armor"] = r.integers(0, 13, 5); rec["target"] = r.integers(0, n0, 5)
    return 5, rec


def spawn_patch(n0):
    def patch(frame, r):
        cnt, rec = children(frame, n0)
        if cnt: r.spawn_count, r.spawn_payload = cnt, rec
    return patch


# ---- request lists and the oracle's sessions --------------------------------------------------------------------------------------------------------------------
# The SyncTest inputs.  k advances by 2 + input per frame (the frame and the Clock), for every entity alike; an own remove and a remote insert of Stun meet in one
# frame only where an insert at frame F (k % 3 == 0) is followed by four frames without one and a fifth with one -- the default's 5 ticks.  (9 t + 15) & 15 has such
# windows inside 14 ticks; the per-feature suites' (5 t + 3) & 15 has none.
INPUTS = lambda t: ((t * 9 + 15) & 15,)      # noqa: E731


def session_lists(n, cd, ticks, with_spawn=False):
    """[(confirmed or None, requests)]: cd >= 0 a SyncTest session of `ticks` ticks, cd < 0 P2P-shaped rollbacks of 0 to 7 frames whose inputs change between
    prediction and confirmation (reduces_common.p2p_lists).  Every AdvanceFrame carries dt explicitly."""
    if cd < 0: return rd.p2p_lists(ticks)
    return [(None, reqs) for reqs in rd.stamp(synctest_lists(cd, ticks, depth=DEPTH, patch=spawn_patch(n) if with_spawn else None, inputs=INPUTS))]


def ring_states(w, ids, resources=False):
    """Every frame the ring holds, loaded newest first (a Load pops the newer snapshots): the state and -- a library world -- the resources the Load restored."""
    out = {}
    for f in reversed([f for f in range(w.frame + 1) if w.has_snapshot(f)]):
        w.load(f)
        out[f] = (cm.snapshot_state(w, ids), sc.read_resources(w, 4) if resources else None)
    return out


class Session:
    """An oracle session with the model beside it: checksums [(frame, oracle ^ resource parts)], the resource words after every list, the final state, {frame: state}
    of the ring, the model and the Stats."""


@functools.lru_cache(maxsize=None)
def oracle_session(n, cd, ticks, kinds=ALL, with_spawn=False):
    o = OracleWorld(n + 128, DEPTH, FLAT); model = skirmish_model(kinds, n + 128); st = Stats()
    ids = build_skirmish(o, kinds, with_spawn=with_spawn, model=model, st=st); spawn_skirmish(o, ids, n); o.set_depth(DEPTH)
    s = Session()
    s.cks, s.per_list, s.st, s.model, s.n = [], [], st, model, n
    for confirmed, reqs in session_lists(n, cd, ticks, with_spawn):
        rd.run_model(o, model, reqs, cd=cd, confirmed=confirmed, got=s.cks)
        s.per_list.append(model.words())
    s.final = cm.snapshot_state(o, ids)
    s.ring = {f: state for f, (state, _) in ring_states(o, ids).items()}      # (rewinds the oracle world: the last thing done with it)
    return s
