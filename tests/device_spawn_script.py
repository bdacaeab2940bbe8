"""The script world: device-decided spawns (e.spawn(n), GGRS_SPAWN_PAYLOAD_PARENT) in which every entity carries its own trigger frame and child count IN DATA, so a
test states exactly who spawns what and when (test_gpu_device_spawn_edges.py), and the oracle side of it with deliberately wrong restatements to hold those tests
against (test_fuzz_device_spawn.py).

Components, in registration order: Plan {at u32, n i32, delta u32, cn u32}, Plan2 {at u32, n i32} (outside the children's bundle), Mix (two 8-byte words), N16 (one
2-byte word), N8 (one 1-byte word).  A system fires for an entity in the frame f.frame == at and calls e.spawn(n) with n AS STORED (negative and above 255 included: the
device clamps, the oracle callback restates the clamp); nobody despawns.  The systems a world registers, in order, are named by `systems`:
  A4   binds Plan (4 bindings, tail zero)
  A8   binds Plan, Mix.0, N16.0, N8.0, Mix.1 -- exactly 8 bindings of 4, 8, 2 and 1 bytes; it churns the narrow words every frame, leaves N16.0 above its width every
       frame and N8.0 above its width in the call that fires (the record holds the raw u64s, the columns the wrapped bytes)
  A3   binds Plan.at, Plan.n, N16.0 (3 bindings)
  B    binds Plan2.at, Plan2.n, Mix.0, N8.0; registered behind an A: it calls for entities A may have called for
The child system binds Plan, Mix.0, Mix.1, N16.0, N8.0 (8 bindings) and folds all 8 record words and k into Mix, N16 and N8; its Plan is read from record words 2 and
3 (under A4 / A8 the parent's delta and cn): at = frame + delta (never, if delta is 0), n = cn, and the same delta and cn again -- so children fire `delta` frames after
their parents, step after step.
(A helper module, no tests of its own.)"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
from fuzz_device_spawn import GOLD, M32, M64, PARENT, U8, U16, U32, U64, fold

NEVER = 0xFFFFFFFF
A4_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    if ((unsigned)f.frame == e.u32(0)) e.spawn(e.i32(1));
}
"""
A8_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    e.u64(4) += 0x100000001ull;
    e.u64(5) = e.u64(5) + 0x1FFFFull;                                           // a 2-byte word left above its width
    e.u8(6) = (unsigned char)(e.u8(6) + 1u);
    e.u64(7) ^= e.u64(4);
    if ((unsigned)f.frame == e.u32(0)) { e.u64(6) = e.u64(6) + 0x300ull; e.spawn(e.i32(1)); }     // ... and a 1-byte word, in the call that fires
}
"""
A3_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    e.u16(2) = (unsigned short)(e.u16(2) * 5u + 1u);
    if ((unsigned)f.frame == e.u32(0)) e.spawn(e.i32(1));
}
"""
B_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    e.u8(3) = (unsigned char)(e.u8(3) + 7u);
    if ((unsigned)f.frame == e.u32(0)) e.spawn(e.i32(1));
}
"""
CHILD_SRC = r"""
__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64 k, const GgrsFrame& f, const unsigned char* payload) {
    const ggrs_u64* p = (const ggrs_u64*)payload;
    ggrs_u64 m = k + 1ull;
    for (int i = 0; i < 8; ++i) m = (m ^ p[i]) * 0x9E3779B97F4A7C15ull + (m >> 29);
    const unsigned d = (unsigned)p[2];
    e.u32(0) = d ? (unsigned)f.frame + d : 0xFFFFFFFFu;
    e.u32(1) = (unsigned)p[3]; e.u32(2) = d; e.u32(3) = (unsigned)p[3];
    e.u64(4) = m;
    e.u64(5) = m ^ (e.slot << 32) ^ k;
    e.u64(6) = m >> 7;                                                          // above the width of a 2-byte word
    e.u64(7) = m >> 11;                                                         // ... and of a 1-byte word
}
"""
HIP_SRC = {"A4": A4_SRC, "A8": A8_SRC, "A3": A3_SRC, "B": B_SRC}
PERTURBATIONS = ("k", "slot", "word", "narrow", "tail", "later", "clamp")


def _clamped(word, perturb):
    """e.spawn(n) of a stored i32, as the device clamps it."""
    v = word & M32
    if v >= 1 << 31: v -= 1 << 32
    return min(max(v, 0), 254 if perturb == "clamp" else 255)


def oracle_systems(perturb=None):
    """The systems restated for the oracle.  perturb: a deliberately WRONG restatement -- "k": the child's k off by one; "slot": the child's own slot off by one (children placed one slot off); "word": record word 7 dropped; "narrow": record
    word 5 wrapped to 16 bits; "tail": a record word behind the bindings not zero; "later": a later non-zero call does not replace; "clamp": 254 instead of 255."""
    called = set()                                                             # (frame, slot) of an A's non-zero calls, for "later"

    def fire(at, nword, f, slot, later=False):
        if (f.frame & M32) != (at & M32): return 0
        ns = _clamped(nword, perturb)
        if perturb == "later" and ns:
            if later and (f.frame, slot) in called: return 0
            if not later: called.add((f.frame, slot))
        return ns

    def a4(words, slot, f): return list(words), 0, fire(words[0], words[1], f, slot)

    def a8(words, slot, f):
        w = list(words)
        w[4] = (w[4] + 0x100000001) & M64
        w[5] = w[5] + 0x1FFFF
        w[6] = (w[6] + 1) & 0xFF
        w[7] ^= w[4]
        ns = fire(w[0], w[1], f, slot)
        if (f.frame & M32) == (w[0] & M32): w[6] += 0x300
        return w, 0, ns

    def a3(words, slot, f):
        w = list(words)
        w[2] = (w[2] * 5 + 1) & 0xFFFF
        return w, 0, fire(w[0], w[1], f, slot)

    def b(words, slot, f):
        w = list(words)
        w[3] = (w[3] + 7) & 0xFF
        return w, 0, fire(w[0], w[1], f, slot, later=True)

    def child(words, slot, k, f, payload):
        p = C.cast(payload, C.POINTER(C.c_uint64))
        pw = [int(p[i]) for i in range(8)]
        if perturb == "word": pw[7] = 0
        if perturb == "narrow": pw[5] &= 0xFFFF
        if perturb == "tail": pw[5] |= 1
        if perturb == "k": k += 1
        if perturb == "slot": slot += 1
        m = fold(pw, k)
        d = pw[2] & M32
        return [((f.frame + d) & M32) if d else NEVER, pw[3] & M32, d, pw[3] & M32, m, m ^ ((slot << 32) & M64) ^ k, m >> 7, m >> 11]
    return {"A4": a4, "A8": a8, "A3": a3, "B": b}, child


@dataclass
class Script:
    """One scripted session: a world of `n` entities, whose Plan / Plan2 rows are NEVER / 0 except for `parents` {slot: (at, n, delta, cn)} and `parents2`
    {slot: (at, n)}, and the steps to play: ("list", requests), ("overflow", requests) -- a list the library must answer with GGRS_E_CAPACITY --, ("state",),
    ("spawn", count) -- a host-side spawn between two lists."""
    capacity: int
    n: int
    systems: tuple = ("A4",)
    parents: dict = field(default_factory=dict)
    parents2: dict = field(default_factory=dict)
    steps: list = field(default_factory=list)
    max_depth: int = 8


def is_hip(w): return isinstance(w, bg.World)


def build(w, sc, perturb=None):
    plan, plan2, mix, n16, n8 = (w.register_component("Plan", 4, 4), w.register_component("Plan2", 4, 2), w.register_component("Mix", 8, 2),
                                 w.register_component("N16", 2, 1), w.register_component("N8", 1, 1))
    ids = (plan, plan2, mix, n16, n8)
    for c, nw in zip(ids, (4, 2, 2, 1, 1)): w.checksum_component(c, list(range(nw)))
    p4 = [(plan, 0), (plan, 1), (plan, 2), (plan, 3)]
    binds = {"A4": p4, "A8": p4 + [(mix, 0), (n16, 0), (n8, 0), (mix, 1)], "A3": [(plan, 0), (plan, 1), (n16, 0)], "B": [(plan2, 0), (plan2, 1), (mix, 0), (n8, 0)]}
    fns, child = (HIP_SRC, CHILD_SRC) if is_hip(w) else oracle_systems(perturb)
    for name in sc.systems: w.add_custom_system(fns[name], binds[name], name=name)
    w.add_spawn_system(child, [plan, mix, n16, n8], p4 + [(mix, 0), (mix, 1), (n16, 0), (n8, 0)], payload_stride=PARENT, name="child")
    n = sc.n
    i = np.arange(n, dtype=np.int64)
    P = np.zeros((4, n), dtype=U32); P[0] = NEVER
    for s, row in sc.parents.items(): P[:, s] = [x & M32 for x in row]
    P2 = np.zeros((2, n), dtype=U32); P2[0] = NEVER
    for s, row in sc.parents2.items(): P2[:, s] = [x & M32 for x in row]
    w.spawn(n, {plan: list(P), plan2: list(P2), mix: [(i.astype(U64) + U64(0x1234567)) << U64(32), i.astype(U64) * U64(GOLD)],
                n16: [((i * 7) & 0xFFFF).astype(U16)], n8: [((i * 3) & 0xFF).astype(U8)]})
    w.set_depth(sc.max_depth)
    if hasattr(w, "set_synctest_check_distance"): w.set_synctest_check_distance(-1)
    return ids


def play(w, sc, perturb=None):
    """Plays the script on a library world or an oracle world; returns what is compared: per step the checksums / frame / len or the state, and the final state."""
    ids = build(w, sc, perturb)
    out = []
    for step in sc.steps:
        if step[0] == "state": out.append(_plain(cm.snapshot_state(w, ids)))
        elif step[0] == "spawn":                                                # the host spawns step[1] entities that never fire (Plan and Mix only)
            k = step[1]
            w.spawn(k, {ids[0]: [np.full(k, NEVER, dtype=U32)] + [np.zeros(k, dtype=U32) for _ in range(3)], ids[2]: [np.full(k, 7, dtype=U64), np.full(k, 9, dtype=U64)]})
            out.append(([], w.frame, w.len))
        elif step[0] == "overflow" and is_hip(w):
            with pytest.raises(bg.GgrsHipError) as e: w.handle_requests(step[1])
            assert e.value.code == bg.GGRS_E_CAPACITY and "capacity" in str(e.value), e.value
            out.append(([], w.frame, w.len))
        else: out.append((list(w.handle_requests(step[1])), w.frame, w.len))
    out.append(_plain(cm.snapshot_state(w, ids)))
    return out


def _plain(state): return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in state.items()}


# ---- request lists -----------------------------------------------------------------------------------------------------------------------------------------------
S, L, A = bg.SaveGameState, bg.LoadGameState, bg.AdvanceFrame


def adv(): return A((0,))


def forward(f, steps):
    """[S f, A, S f+1, A, ..]: `steps` AdvanceFrames from frame f, a Save ahead of each."""
    return [q for k in range(steps) for q in (S(f + k), adv())]


def synctest(f0, steps):
    """[L f0, A, S, A, S, .., A]: a SyncTest tick that re-simulates steps - 1 frames and then advances."""
    return [L(f0)] + [q for k in range(steps - 1) for q in (adv(), S(f0 + k + 1))] + [adv()]


# ---- the scripts -------------------------------------------------------------------------------------------------------------------------------------------------
LENS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513)
COUNTS = (1, 2, 255)


def len_edge(n, c):
    """One parent at slot 0 and one at slot len - 1 (with the next count of COUNTS), both in frame 1; the first parent's children spawn one each in frame 2.  Then the
    two frames again inside one list, behind Loads."""
    c2 = COUNTS[(COUNTS.index(c) + 1) % 3]
    parents = {0: (1, c, 1, 1)}
    if n > 1: parents[n - 1] = (1, c2, 0, 0)
    steps = [("list", forward(0, 2) + [S(2)]), ("state",), ("list", [L(0), adv(), S(1), adv(), S(2), L(1), adv(), S(2)])]
    return Script(1100, n, parents=parents, steps=steps)


def three_fans_in_one_tile():
    return Script(1100, 300, parents={3: (1, 255, 0, 0), 100: (1, 255, 0, 0), 255: (1, 255, 0, 0)}, steps=[("list", forward(0, 2) + [S(2)])])


def fans_across_empty_tiles():
    """Parents at slots 0, 300 and 700 of 720: tiles 1 has one parent, tile 0 one, tile 2 one at its end; their children (200, 255, 100) start at 720 and straddle
    slots 768, 1024 and 1280; in frame 2 two more parents, with tiles between them that hold children but no parent."""
    parents = {0: (1, 200, 0, 0), 300: (1, 255, 0, 0), 700: (1, 100, 0, 0), 1: (2, 7, 0, 0), 301: (2, 255, 0, 0)}
    return Script(1600, 720, parents=parents, steps=[("list", forward(0, 2) + [S(2)]), ("state",), ("list", synctest(0, 3))])


def exact_fit(capacity, short=0):
    """312 children (255 + 57) into a world of capacity - 312 entities: len + total == capacity.  short=1: the world has one slot fewer; the frame's spawns are
    dropped, GGRS_E_CAPACITY is reported for a list that holds that AdvanceFrame alone, and the next list -- with a frame that spawns 3 -- goes on from there."""
    n = capacity - 312
    parents = {5: (1, 255, 0, 0), n - 50: (1, 57, 0, 0), 7: (2, 3, 0, 0)}
    if short: return Script(capacity - 1, n, parents=parents, steps=[("list", [S(0)]), ("overflow", [adv()]), ("state",), ("list", [S(1), adv(), S(2)])])
    parents.pop(7)
    return Script(capacity, n, parents=parents, steps=[("list", [S(0)]), ("list", [adv()]), ("state",), ("list", [S(1), adv(), S(2)])])


CHAIN_DEPTH = 4                                                                 # max_depth of the chain worlds: their groups end at 5 Saves / 6 steps


def chain(steps):
    """Every step of a SyncTest-shaped list spawns, and the children of step s spawn in step s + 1: the root has 3 children, every child 2."""
    return Script(1700, 5, parents={2: (1, 3, 1, 2)}, max_depth=CHAIN_DEPTH, steps=[("list", [S(0)]), ("list", synctest(0, steps)), ("state",), ("list", forward(steps, 2))])


def many_launches():
    """22 lists of one AdvanceFrame each, alternately [S, A] and [A, S]; a new parent every frame and every child spawns one child in the next frame, so every launch
    spawns -- on both sides of the 9th and the 18th."""
    parents = {i: (i + 1, 1 + i % 3, 1, 1) for i in range(22)}
    steps = [("list", [S(f), adv()] if f % 2 == 0 else [adv(), S(f + 1)]) for f in range(22)]
    return Script(1500, 64, parents=parents, steps=steps + [("list", [S(22)])])


def saves_alone():
    """Lists that hold Saves only: the world's FIRST list, and one behind a host-side spawn.  Such a launch does not write the live world, so the device's copy of
    RollbackOrdered::len is not written either: the host's len must stand (it read 0 after the first, and lost the host's spawns after the second)."""
    steps = [("list", [S(0)]), ("list", [adv(), S(1)]), ("spawn", 5), ("list", [S(1)]), ("state",), ("list", [adv(), S(2), adv()])]
    return Script(300, 70, parents={3: (1, 4, 1, 2)}, steps=steps)


def record(system):
    """A8: exactly 8 bindings of four widths; A3: three, the tail zero."""
    return Script(300, 70, systems=(system,), parents={3: (1, 3, 1, 1), 69: (2, 2, 1, 1)}, steps=[("list", forward(0, 3) + [S(3)])])


def two_callers():
    """Frame 1.  Slot 2: A asks for 3, B for 2 -- B's call wins, with B's record.  Slot 10: A asks for 3, B calls e.spawn(0) -- A's call stands, with A's record.
    Slot 20: A calls e.spawn(0), B asks for 4.  Slot 30: A asks for 2, B for -1.  Slot 40: B alone."""
    return Script(300, 70, systems=("A4", "B"), parents={2: (1, 3, 0, 0), 10: (1, 3, 0, 0), 20: (1, 0, 0, 0), 30: (1, 2, 0, 0)},
                  parents2={2: (1, 2), 10: (1, 0), 20: (1, 4), 30: (1, -1), 40: (1, 5)}, steps=[("list", forward(0, 2) + [S(2)])])


def clamps():
    """e.spawn(-3) gives none and e.spawn(1000) gives 255 (frame 1); e.spawn(256) gives 255 and e.spawn(INT_MIN) none (frame 2)."""
    return Script(700, 70, parents={1: (1, -3, 0, 0), 2: (1, 1000, 0, 0), 3: (2, 256, 0, 0), 4: (2, -(1 << 31), 0, 0)}, steps=[("list", forward(0, 2) + [S(2)])])


# every script by name, and a wrong restatement under which its comparison must fail (test_fuzz_device_spawn.py shows it on the CPU)
SCRIPTS = {f"len{n}x{c}": (lambda n=n, c=c: len_edge(n, c), "slot") for n in LENS for c in COUNTS}
SCRIPTS.update({"three_fans": (three_fans_in_one_tile, "slot"), "fans_across": (fans_across_empty_tiles, "slot"),
                "fit512": (lambda: exact_fit(512), "k"), "fit519": (lambda: exact_fit(519), "k"), "short512": (lambda: exact_fit(512, 1), "k"), "short519": (lambda: exact_fit(519, 1), "k"),
                "chain6": (lambda: chain(6), "k"), "chain7": (lambda: chain(7), "k"), "launches": (many_launches, "k"), "saves_alone": (saves_alone, "k"),
                "record8": (lambda: record("A8"), "word"), "record8_narrow": (lambda: record("A8"), "narrow"), "record3": (lambda: record("A3"), "tail"),
                "two_callers": (two_callers, "later"), "clamps": (clamps, "clamp")})
