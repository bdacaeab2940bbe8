"""The worlds of the command-binding tests (ggrs_hip_add_custom_system_commands: a user-written system inserts and removes components of its OWN entity), each built
twice: on a library world from HIP C++ source, and on the CPU oracle (oracle.binding.OracleWorld, unchanged) from Python callbacks.

The oracle's custom-system callback cannot insert or remove.  But its loop is serial (one system after the other, one entity after the other, FLAT mode), and
insert_component / remove_component / upload_word may be called on the same world from inside the callback: a callback bound to the system's OWN words looks the
entity's command-bound component up in a cache taken at the start of its pass (nothing but the entity's own call changes it during the pass) and edits the world
directly.  Every mirror counts its inserts, removes and in-place writes (Counts): a parity test asserts that each happened.

    stun      Hp 1 x u32 (checksummed); Stun {ticks, seed} 2 x u32 (checksummed), absent at spawn.  ONE system, own binding Hp, command binding Stun with
              INSERT | REMOVE: hp += input; a stunned entity counts down and loses Stun at 1; any other whose (hp + slot) % 5 == 0 gains Stun{3, hp}; a few
              entities despawn themselves in the call that inserts (`kills`).
    shield    Hp 1 x u32; Shield {charge} 1 x u64 (8-byte word), both checksummed; every fourth entity has Shield at spawn.
                drain    (EARLIER) own binding Shield.charge: charge -= 1 -- an entity that gains Shield in frame f is drained from frame f + 1 on
                granter  own binding Hp, command binding Shield with INSERT | REMOVE
                absorb   own binding Hp, command binding Shield with flags 0 -- Option<&mut Shield>: has() and a write in place, no command
                tally    (LATER) own bindings Shield.charge and Hp: runs in the SAME frame for an entity that just gained Shield
    watch     the stun world with Target 1 x u64 and Seen 1 x u32 in front: `watcher`, registered FIRST, peer-reads Stun.ticks of its target, which the LATER
              stun system inserts: ok() follows the presence at the start of the frame
(A helper module, no tests of its own.)"""
import numpy as np

import bevy_ggrs_amd as bg
from oracle.binding import OracleWorld
from peer_effects_common import _Pass, run_oracle, synctest_lists  # noqa: F401  (re-exported: the list builders the tests share)

U32, U64 = np.uint32, np.uint64
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
BOTH = bg.CMD_INSERT | bg.CMD_REMOVE

# binding 0 = Hp; command binding 0 = Stun {ticks, seed}.  iparam[0] != 0: an entity whose slot % 29 == 7 despawns itself in the call that inserts
STUN_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    e.u32(0) = e.u32(0) + (ggrs_u32)f.input[0];
    if (e.has(0)) {
        if (e.opt_u32(0, 0) <= 1u) e.remove(0);
        else e.opt_u32(0, 0) -= 1u;
    } else if ((e.u32(0) + (ggrs_u32)e.slot) % 5u == 0u) {
        e.opt_u32(0, 0) = 3u; e.opt_u32(0, 1) = e.u32(0);
        e.insert(0);
        if (f.iparam[0] && e.slot % 29ull == 7ull) e.despawn();          // commands apply even when the same call despawns the entity
    }
}
"""
# the comparison world of scripts/bench_commands.py: Stun always present, the same arithmetic through ordinary bindings (1 = ticks, 2 = seed); the masks never change
STUN_OWN_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    e.u32(0) = e.u32(0) + (ggrs_u32)f.input[0];
    if (e.u32(1)) {
        if (e.u32(1) <= 1u) e.u32(1) = 0u;
        else e.u32(1) -= 1u;
    } else if ((e.u32(0) + (ggrs_u32)e.slot) % 5u == 0u) {
        e.u32(1) = 3u; e.u32(2) = e.u32(0);
    }
}
"""
STUN_CHILD_SRC = r"""
__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64 k, const GgrsFrame& f, const unsigned char*) { e.u32(0) = 1000u + 7u * (ggrs_u32)k + (ggrs_u32)f.frame; }
"""
STUN_CHILD_WITH_SRC = r"""
__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64 k, const GgrsFrame& f, const unsigned char*) { e.u32(0) = 1000u + 7u * (ggrs_u32)k + (ggrs_u32)f.frame; e.u32(1) = 2u + (ggrs_u32)(k & 1ull); }
"""
DRAIN_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u64(0) = e.u64(0) - 1ull; }"
GRANT_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u32 k = e.u32(0) + (ggrs_u32)e.slot + (ggrs_u32)f.frame;
    if (!e.has(0)) {
        if (k % 7u == 0u) { e.opt_u64(0, 0) = 0x500000000ull + e.u32(0); e.insert(0); }
    } else if ((e.opt_u64(0, 0) & 0xFFull) < 6ull || k % 11u == 0u) e.remove(0);
}
"""
ABSORB_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    e.u32(0) = e.u32(0) + (ggrs_u32)f.input[0];
    if (e.has(0)) e.opt_u64(0, 0) = e.opt_u64(0, 0) + 0x100000000ull + (e.u32(0) & 3u);
}
"""
TALLY_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(1) = e.u32(1) + (ggrs_u32)(e.u64(0) >> 32); }"
# binding 0 = Target, 1 = Seen; peer binding 0 = Stun.ticks
WATCH_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) {
    const GgrsPeer p = e.peer(e.u64(0));
    e.u32(1) = e.u32(1) + (p.ok() ? 1u + p.u32(0) : 100u);
}
"""


class Counts:
    def __init__(self): self.inserts = self.removes = self.writes = 0


class _Cache(_Pass):
    """The command-bound component of every slot at the start of the current pass of one oracle system: presence and words."""

    def refresh(self, o, comp, n_words, slot, frame):
        if self.begin(slot, frame):
            n = o.len
            self.has = o.present_mask(comp, n).tolist()
            self.w = [o.download_word(comp, k, 0, n).tolist() for k in range(n_words)]


def _stun_fn(o, S, cnt, kills):
    c = _Cache()

    def stun(words, slot, f):
        c.refresh(o, S, 2, slot, f.frame)
        hp = (words[0] + f.input(0)[0]) & M32
        kill = 0
        if c.has[slot]:
            if c.w[0][slot] <= 1: o.remove_component(S, slot); cnt.removes += 1
            else: o.upload_word(S, 0, slot, np.array([c.w[0][slot] - 1], dtype=U32)); cnt.writes += 1
        elif (hp + slot) % (1 << 32) % 5 == 0:
            o.insert_component(S, slot, np.array([3, hp], dtype=U32)); cnt.inserts += 1
            if kills and slot % 29 == 7: kill = 1
        return [hp], kill
    return stun


def build_stun(w, *, kills=False, spawn=None, cnt=None):
    """Registers the stun world on `w` (a library world or the oracle); returns (Hp, Stun).  spawn: None, "without" or "with" -- a user-written spawn system
    (host-decided counts) whose bundle excludes or includes Stun."""
    H = w.register_component("Hp", 4, 1); S = w.register_component("Stun", 4, 2)
    w.set_component_default(S, np.array([9, 77], dtype=U32))                 # (never seen: an absent entity's opt words are overwritten before the insert)
    w.checksum_component(H, [0]); w.checksum_component(S, [0, 1])
    bundle = (H, S) if spawn == "with" else (H,)
    binds = [(H, 0), (S, 0)] if spawn == "with" else [(H, 0)]
    if isinstance(w, OracleWorld):
        w.add_custom_system(_stun_fn(w, S, cnt if cnt is not None else Counts(), kills), [(H, 0)], iparam=(int(kills), 0))
        if spawn:
            def child(words, slot, k, f, payload):
                return [(1000 + 7 * k + f.frame) & M32] + ([2 + (k & 1)] if spawn == "with" else [])
            w.add_spawn_system(child, bundle=bundle, bindings=binds)
    else:
        w.add_custom_system(STUN_SRC, [(H, 0)], iparam=(int(kills), 0), name="stun", commands=[(S, BOTH)])
        if spawn: w.add_spawn_system(STUN_CHILD_WITH_SRC if spawn == "with" else STUN_CHILD_SRC, bundle=bundle, bindings=binds, name="child")
    return H, S


def spawn_stun(w, ids, n):
    w.spawn(n, {ids[0]: [((np.arange(n) * 37 + 11) % 101).astype(U32)]})


def build_shield(w, *, cnt=None):
    """Registers the shield world; returns (Hp, Shield)."""
    H = w.register_component("Hp", 4, 1); S = w.register_component("Shield", 8, 1)
    w.set_component_default(S, np.array([0xABCD00000000], dtype=U64))
    w.checksum_component(H, [0]); w.checksum_component(S, [0])
    if isinstance(w, OracleWorld):
        cnt = cnt if cnt is not None else Counts()
        cg, ca = _Cache(), _Cache()

        def drain(words, slot, f): return [(words[0] - 1) & M64], 0

        def grant(words, slot, f):
            cg.refresh(w, S, 1, slot, f.frame)
            k = (words[0] + slot + f.frame) & M32
            if not cg.has[slot]:
                if k % 7 == 0: w.insert_component(S, slot, np.array([0x500000000 + words[0]], dtype=U64)); cnt.inserts += 1
            elif (cg.w[0][slot] & 0xFF) < 6 or k % 11 == 0: w.remove_component(S, slot); cnt.removes += 1
            return [words[0]], 0

        def absorb(words, slot, f):
            ca.refresh(w, S, 1, slot, f.frame)                                  # (taken after the granter's pass: this frame's inserts and removes are in)
            hp = (words[0] + f.input(0)[0]) & M32
            if ca.has[slot]: w.upload_word(S, 0, slot, np.array([(ca.w[0][slot] + 0x100000000 + (hp & 3)) & M64], dtype=U64)); cnt.writes += 1
            return [hp], 0

        def tally(words, slot, f): return [words[0], (words[1] + (words[0] >> 32)) & M32], 0
        w.add_custom_system(drain, [(S, 0)]); w.add_custom_system(grant, [(H, 0)]); w.add_custom_system(absorb, [(H, 0)]); w.add_custom_system(tally, [(S, 0), (H, 0)])
    else:
        w.add_custom_system(DRAIN_SRC, [(S, 0)], name="drain")
        w.add_custom_system(GRANT_SRC, [(H, 0)], name="granter", commands=[(S, BOTH)])
        w.add_custom_system(ABSORB_SRC, [(H, 0)], name="absorb", commands=[(S, 0)])
        w.add_custom_system(TALLY_SRC, [(S, 0), (H, 0)], name="tally")
    return H, S


def spawn_shield(w, ids, n):
    """Blocks of four: the first of each block has Shield at spawn (charges around the granter's removal threshold)."""
    H, S = ids
    i = np.arange(n)
    hp = ((i * 13 + 5) % 97).astype(U32)
    for first in range(0, n, 4):
        m = min(4, n - first)
        w.spawn(1, {H: [hp[first:first + 1]], S: [np.array([0x300000000 + (first % 23)], dtype=U64)]})
        if m > 1: w.spawn(m - 1, {H: [np.ascontiguousarray(hp[first + 1:first + m])]})


def build_watch(w, *, cnt=None):
    """Registers the watch world; returns (Target, Seen, Hp, Stun)."""
    T = w.register_component("Target", 8, 1); N = w.register_component("Seen", 4, 1)
    H = w.register_component("Hp", 4, 1); S = w.register_component("Stun", 4, 2)
    w.set_component_default(S, np.array([9, 77], dtype=U32))
    for c, words in ((T, [0]), (N, [0]), (H, [0]), (S, [0, 1])): w.checksum_component(c, words)
    if isinstance(w, OracleWorld):
        pw = _Pass()

        def watch(words, slot, f):
            if pw.begin(slot, f.frame):
                n = w.len
                pw.vis = (w.alive_mask(n) & w.present_mask(S, n)).tolist()     # the peer view at the start of the frame (the watcher is the first system)
                pw.ticks, pw.n = w.download_word(S, 0, 0, n).tolist(), n
            t = words[0]
            ok = t < pw.n and pw.vis[t]
            return [t, (words[1] + (1 + pw.ticks[t] if ok else 100)) & M32], 0
        w.add_custom_system(watch, [(T, 0), (N, 0)])
        w.add_custom_system(_stun_fn(w, S, cnt if cnt is not None else Counts(), False), [(H, 0)])
    else:
        w.add_custom_system(WATCH_SRC, [(T, 0), (N, 0)], name="watcher", peers=[(S, 0)])
        w.add_custom_system(STUN_SRC, [(H, 0)], name="stun", commands=[(S, BOTH)])
    return T, N, H, S


def spawn_watch(w, ids, n):
    T, N, H, S = ids
    i = np.arange(n, dtype=U64)
    link = (i * U64(389) + U64(17)) % U64(n)
    link[i % U64(10) == 3] = n + 5                                          # out of range: never ok()
    w.spawn(n, {T: [link], N: [np.zeros(n, dtype=U32)], H: [((np.arange(n) * 37 + 11) % 101).astype(U32)]})
