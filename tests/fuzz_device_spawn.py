"""The colony world: device-decided spawns (e.spawn(n), GGRS_SPAWN_PAYLOAD_PARENT) as a scenario of the request fuzzer (fuzz_util.run(scenario=...)),
and its oracle side as one backend object (the OracleAdapter / InFlight pattern of fuzz_user_worlds.py).

Components, in registration order: Cell {x f32, v f32, fuse u32, gen u32}; a 1-byte Tag that is OUTSIDE the children's bundle and bound by no system; Wide (two 8-byte
words) and Half (two 2-byte words), both inside the bundle.  One entity in eight starts without Half.

Systems:
  * split   binds all of Cell (4 bindings: the record's tail is zero).  The cell drifts, its fuse burns; when the fuse runs out a cell with gen < max_gen calls
            e.spawn(k), k = a hash of slot, gen, frame and the AdvanceFrame's input byte in 0 .. maxk -- so e.spawn(0) happens and a frame re-advanced with another
            input splits differently -- and despawns.  One firing cell in four is HANDED ON instead: split sets bit 8 of gen (the cell can never pass gen < max_gen
            again) and leaves the despawn to relay.
  * relay   registered behind split; binds (Wide.0, Half.0, Cell.fuse, Cell.gen, Half.1): 8-, 2- and 4-byte words, 5 bindings.  It churns its narrow words every
            frame -- Half.1 is left ABOVE its width (the record holds the raw u64, the column the wrapped 16 bits) -- and for a handed-on cell calls e.spawn(k2) with k2
            in -1 .. maxk and despawns: a k2 > 0 replaces split's call with relay's record, k2 <= 0 leaves split's call standing (-1 is clamped to 0).
  * child   folds all 8 payload words and k into every word of the child, so a stale or un-zeroed record word shows in the checksum; gen = the parent's + 1; three
            children in four get a fuse of 1 .. 3 (they fire inside the group that made them), the rest 4 .. 12.

THE BOUND.  A cell calls e.spawn at most once in any timeline with an effect: afterwards it is dead or carries bit 8, which relay or split's next pass turns into a
despawn.  The host only ever writes gen as max_gen (words()), so it cannot re-arm a lineage, and len <= n * (1 + maxk + .. + maxk^max_gen) whatever is rolled back.
The capacity is that bound plus a slack, never a multiple of 256, far below the resident form's limit.  The adapter counts, per AdvanceFrame, the children the
callbacks asked for (the last non-zero call per entity) and the child callbacks that ran: equal in every frame means no frame ever met the capacity.
(A helper module, no tests of its own.)"""
import ctypes as C

import numpy as np

import bevy_ggrs_amd as bg
import fuzz_user_worlds as fu
import fuzz_util
from oracle.binding import FLAT, REFSHAPED, OracleWorld

U8, U16, U32, U64, F32 = np.uint8, np.uint16, np.uint32, np.uint64, np.float32
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
PARENT = 0xFFFFFFFF                                              # GGRS_SPAWN_PAYLOAD_PARENT
HANDED = 0x100                                                   # bit 8 of gen: split fired and left the despawn to relay
GOLD, LCG_A, LCG_C = 0x9E3779B97F4A7C15, 6364136223846793005, 1442695040888963407
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025)
BOUND_MAX = 8000                                                 # slots: the oracle calls Python once per entity, system and frame
RUN_KW = fu.RUN_KW
CAP_SAVES, CAP_STEPS = 9, 10                                      # kernel_info()["group_caps"] of a world of max_depth 8: max_depth + 1 Saves / + 2 steps

HASH_SRC = r"""
static __device__ unsigned colony_hash(unsigned a, unsigned b, unsigned c, unsigned d) {
    unsigned h = (a * 2654435761u) ^ (b * 40503u) ^ (c * 2246822519u) ^ (d * 3266489917u);
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    return h;
}
"""
SPLIT_SRC = HASH_SRC + r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    e.f32(0) = e.f32(0) + e.f32(1) * f.dt;
    if (e.u32(2) > 0u) e.u32(2) -= 1u;
    if (e.u32(2) == 0u) {
        if (e.u32(3) < (unsigned)f.iparam[0]) {
            const unsigned h = colony_hash((unsigned)e.slot, e.u32(3), (unsigned)f.frame, (unsigned)f.input[0]);
            e.spawn((int)((h >> 8) % ((unsigned)f.iparam[1] + 1u)));
            if ((h & 3u) == 0u) { e.u32(3) |= 0x100u; return; }                 // handed on: relay despawns it (and may call e.spawn again)
        }
        e.despawn();
    }
}
"""
RELAY_SRC = HASH_SRC + r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    e.u64(0) = e.u64(0) * 6364136223846793005ull + 1442695040888963407ull;
    e.u16(1) = (unsigned short)(e.u16(1) + 3u);
    e.u64(4) = e.u64(4) + 0x1FFFFull;                                           // a 2-byte word left above its width
    if (e.u32(2) == 0u && (e.u32(3) & 0x100u) != 0u) {
        const unsigned gen = e.u32(3) & 0xFFu;
        const unsigned h = colony_hash((unsigned)e.slot ^ 0x5bd1e995u, gen, (unsigned)f.frame, (unsigned)f.input[0]);
        e.u32(3) = gen;
        e.spawn((int)(h % ((unsigned)f.iparam[1] + 2u)) - 1);                   // -1 .. maxk
        e.despawn();
    }
}
"""
CHILD_SRC = r"""
__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64 k, const GgrsFrame& f, const unsigned char* payload) {
    const ggrs_u64* p = (const ggrs_u64*)payload;
    ggrs_u64 m = k + 1ull;
    for (int i = 0; i < 8; ++i) m = (m ^ p[i]) * 0x9E3779B97F4A7C15ull + (m >> 29);
    e.f32(0) = (float)(unsigned)((m >> 40) & 0xFFFFull) * 0.0625f - 2048.0f;
    e.f32(1) = (float)(unsigned)((m >> 24) & 0xFFFull) * 0.125f - 256.0f;
    const unsigned r = (unsigned)(m >> 8) & 0xFFu;
    e.u32(2) = (r & 3u) != 0u ? 1u + r % 3u : 4u + r % 9u;
    e.u32(3) = ((unsigned)p[3] & 0xFFu) + 1u;
    e.u64(4) = m;
    e.u64(5) = p[4] ^ (k << 56) ^ e.slot;
    e.u16(6) = (unsigned short)(m >> 3);
    e.u64(7) = m >> 5;                                                          // above the width of a 2-byte word
}
"""


def f32(x): return np.float32(x)
def bits(x): return int(np.float32(x).view(np.uint32))
def unbits(u): return np.uint32(u & M32).view(np.float32)


def chash(a, b, c, d):
    h = ((a * 2654435761) ^ (b * 40503) ^ (c * 2246822519) ^ (d * 3266489917)) & M32
    h ^= h >> 15; h = (h * 2246822519) & M32; h ^= h >> 13; h = (h * 3266489917) & M32; h ^= h >> 16
    return h


def fold(pw, k):
    m = (k + 1) & M64
    for i in range(8): m = ((m ^ pw[i]) * GOLD + (m >> 29)) & M64
    return m


# ---- the oracle side ---------------------------------------------------------------------------------------------------------------------------------------------
class Counts:
    """What the callbacks and the adapter saw: per AdvanceFrame the calls and the children, over the session what the CPU tier's floors are counted from."""

    def __init__(self):
        self.req, self.first, self.built, self.born = {}, {}, 0, set()
        self.frames = self.mismatches = self.children = self.list_children = 0
        self.spawn0 = self.negative = self.both_called = self.later_won = self.later_zero_kept = self.child_spawned = 0
        self.consecutive_lists = self.load_then_spawn_lists = self.cross64 = self.cross256 = self.cross8192 = 0
        self.totals = {}                                                        # frame -> the child totals of every pass over it

    def call(self, system, slot, n):
        """e.spawn(n) as the device clamps it: a later call replaces an earlier one only when it is non-zero."""
        self.spawn0 += n == 0; self.negative += n < 0
        n = min(max(n, 0), 255)
        if system == 0: self.first[slot] = n
        elif slot in self.first:
            self.both_called += 1; self.later_won += n > 0; self.later_zero_kept += n == 0 and self.first[slot] > 0
        if n:
            self.req[slot] = n
            self.child_spawned += slot in self.born
        return n

    def twice_with_other_totals(self): return sum(len(s) > 1 for s in self.totals.values())

    def floors(self):
        return {"consecutive_lists": self.consecutive_lists, "child_spawned": self.child_spawned, "twice_with_other_totals": self.twice_with_other_totals(),
                "load_then_spawn_lists": self.load_then_spawn_lists, "both_called": self.both_called, "spawn0": self.spawn0, "cross64": self.cross64}


def callbacks(counts, perturb=None):
    """The three systems restated for the oracle.  perturb: a deliberately WRONG restatement ("k": the child's k off by one, "word": record word 6 dropped)."""

    def split(words, slot, f):
        x, v, fuse, gen = unbits(words[0]), unbits(words[1]), words[2] & M32, words[3] & M32
        x = f32(x + f32(v * f32(f.dt)))
        if fuse > 0: fuse -= 1
        kill, ns = 0, 0
        if fuse == 0:
            kill = 1
            if gen < f.iparam[0]:
                h = chash(slot & M32, gen, f.frame & M32, int(f.inputs[0]))
                ns = counts.call(0, slot, (h >> 8) % (f.iparam[1] + 1))
                if h & 3 == 0: gen |= HANDED; kill = 0
        return [bits(x), words[1], fuse, gen], kill, ns

    def relay(words, slot, f):
        w0 = (words[0] * LCG_A + LCG_C) & M64
        h0 = (words[1] + 3) & 0xFFFF
        h1 = words[4] + 0x1FFFF                                                 # raw: the record holds it, the column its low 16 bits
        fuse, gen = words[2] & M32, words[3] & M32
        kill, ns = 0, 0
        if fuse == 0 and gen & HANDED:
            gen &= 0xFF
            h = chash((slot & M32) ^ 0x5bd1e995, gen, f.frame & M32, int(f.inputs[0]))
            ns = counts.call(1, slot, h % (f.iparam[1] + 2) - 1)
            kill = 1
        return [w0, h0, fuse, gen, h1], kill, ns

    def child(words, slot, k, f, payload):
        p = C.cast(payload, C.POINTER(C.c_uint64))
        pw = [int(p[i]) for i in range(8)]
        if perturb == "word": pw[6] = 0
        if perturb == "k": k += 1
        counts.built += 1
        m = fold(pw, k)
        x = f32(f32(f32((m >> 40) & 0xFFFF) * f32(0.0625)) - f32(2048.0))
        v = f32(f32(f32((m >> 24) & 0xFFF) * f32(0.125)) - f32(256.0))
        r = (m >> 8) & 0xFF
        return [bits(x), bits(v), (1 + r % 3) if r & 3 else (4 + r % 9), (pw[3] & 0xFF) + 1, m, pw[4] ^ ((k << 56) & M64) ^ slot, (m >> 3) & 0xFFFF, m >> 5]
    return split, relay, child


class ColonyAdapter(fu.OracleAdapter):
    """An OracleWorld behind the surface fuzz_util.run drives, walked request by request so that every AdvanceFrame's calls and children are counted."""

    def __init__(self, oracle, counts, perturb=None): self.__dict__.update(oracle=oracle, counts=counts, perturb=perturb)

    def handle_requests(self, reqs):
        o, c, out = self.oracle, self.counts, []
        c.born, c.list_children = set(), 0
        prev = lowered = consecutive = load_then_spawn = False
        saves = steps = 0                                                       # of the request group the library is in: it ends at a Load and at CAP_SAVES / CAP_STEPS
        for r in reqs:
            if isinstance(r, bg.SaveGameState):
                if saves == CAP_SAVES: saves, steps, prev = 0, 0, False
                saves += 1
                out += o.handle_requests([r]); continue
            len0 = o.len
            if isinstance(r, bg.LoadGameState):
                o.handle_requests([r])
                lowered |= o.len < len0
                c.born, prev, saves, steps = set(), False, 0, 0                  # (what the slots above hold now is another timeline's)
                continue
            if steps == CAP_STEPS: saves, steps, prev = 0, 0, False
            steps += 1
            c.req, c.first, c.built = {}, {}, 0
            o.handle_requests([r])
            asked, built = sum(c.req.values()), c.built
            c.frames += 1; c.mismatches += asked != built or o.len != len0 + built
            c.totals.setdefault(o.frame, set()).add(built)
            if built:
                c.children += built; c.list_children += built
                consecutive |= prev; load_then_spawn |= lowered
                c.cross64 += len0 > 0 and (len0 + built - 1) >> 6 > (len0 - 1) >> 6
                c.cross256 += len0 > 0 and (len0 + built - 1) >> 8 > (len0 - 1) >> 8
                c.cross8192 += len0 > 0 and (len0 + built - 1) >> 13 > (len0 - 1) >> 13
                c.born |= set(range(len0, len0 + built))
            prev = built > 0
        c.consecutive_lists += consecutive; c.load_then_spawn_lists += load_then_spawn
        return out


class InFlight(fu.InFlight):
    """fuzz_user_worlds.InFlight, and of the enqueued lists that saw a host edit behind them: how many had spawned (spawning_edited)."""

    def __init__(self, w): super().__init__(w); self.__dict__["spawning_edited"] = 0

    def __getattr__(self, k):
        v = fu.InFlight.__getattr__(self, k)
        if k not in fu.EDITS: return v

        def edit(*a, **kw):
            self.__dict__["spawning_edited"] += sum(1 for e in self._q if not e[1] and e[2])
            return v(*a, **kw)
        return edit

    def enqueue_requests(self, reqs):
        cs = list(self._w.handle_requests(reqs))
        self._q.append([cs, False, self._w.counts.list_children > 0])


# ---- the scenario ------------------------------------------------------------------------------------------------------------------------------------------------
def geometric(max_gen, maxk): return sum(maxk ** g for g in range(max_gen + 1))


class ColonyScenario(fu._UserScenario):
    """n from SIZES (or pinned), depth 1..8, (max_gen, maxk) drawn among the shapes whose bound n * (1 + maxk + .. + maxk^max_gen) stays within BOUND_MAX slots
    (two generations and maxk >= 2 where they fit); every AdvanceFrame carries a drawn input byte 0..15.  Host edits are the generator's own, with the words of `cols`: finite floats for
    x and v, fuses 0 .. 39, gen only ever max_gen; and one of its own, `rekindle` (extra_edit)."""
    with_spawn, spawn_budget = False, 0
    #        Cell                       Tag       Wide            Half
    cols = (("f", "f", (0, 40), "gen"), ("u8",), ("u64", "u64"), ("u16", "u16"))

    def __init__(self, seed, n=None):
        r = self.rng = np.random.default_rng([0xC0107, seed])
        self.seed = seed
        drawn = int(r.choice(SIZES))
        self.n = drawn if n is None else n                                      # (a pinned size: every draw is made as usual)
        self.depth = int(r.integers(1, 9))
        fits = [(g, k) for g in (1, 2, 3) for k in (2, 3, 4) if self.n * geometric(g, k) <= BOUND_MAX]
        shapes = [s for s in fits if s[0] >= 2] or fits or [(1, 1)]             # (two generations where they fit: children that become parents)
        self.max_gen, self.maxk = shapes[int(r.integers(len(shapes)))]
        self.bound = self.n * geometric(self.max_gen, self.maxk)
        self.capacity = self.bound + 37
        if self.capacity % 256 == 0: self.capacity += 1

    def describe(self):
        return f"colony seed {self.seed}: n={self.n} max_gen={self.max_gen} maxk={self.maxk} capacity={self.capacity} depth={self.depth}"

    def oracle(self, mode, perturb=None): return ColonyAdapter(OracleWorld(self.capacity, 8, mode), Counts(), perturb)

    def build(self, world):
        w = world.oracle if hasattr(world, "oracle") else world
        cell, tag, wide, half = w.register_component("Cell", 4, 4), w.register_component("Tag", 1, 1), w.register_component("Wide", 8, 2), w.register_component("Half", 2, 2)
        for c, nw in ((cell, 4), (tag, 1), (wide, 2), (half, 2)): w.checksum_component(c, list(range(nw)))
        b_split = [(cell, 0), (cell, 1), (cell, 2), (cell, 3)]
        b_relay = [(wide, 0), (half, 0), (cell, 2), (cell, 3), (half, 1)]
        b_child = b_split + [(wide, 0), (wide, 1), (half, 0), (half, 1)]
        src = (SPLIT_SRC, RELAY_SRC, CHILD_SRC) if w is world else callbacks(world.counts, world.perturb)
        ip = (self.max_gen, self.maxk)
        w.add_custom_system(src[0], b_split, iparam=ip, name="split")
        w.add_custom_system(src[1], b_relay, iparam=ip, name="relay")
        w.add_spawn_system(src[2], [cell, wide, half], b_child, payload_stride=PARENT, name="child")
        n = self.n
        i = np.arange(n, dtype=np.int64)
        cols = {cell: [(((i * 37) % 201 - 100) * 0.25).astype(F32).view(U32), (((i * 11) % 33 - 16) * 0.5).astype(F32).view(U32),
                       (1 + (i * 7 + self.seed) % 61).astype(U32), np.zeros(n, dtype=U32)],
                tag: [(i % 7).astype(U8)],
                wide: [i.astype(U64) * U64(GOLD), i.astype(U64)],
                half: [((i * 3) & 0xFFFF).astype(U16), (65535 - (i & 0xFF)).astype(U16)]}
        a = n - n // 8                                                          # the last eighth has no Half: relay does not run for it
        w.spawn(a, {c: [col[:a] for col in v] for c, v in cols.items()})
        if n - a: w.spawn(n - a, {c: [col[a:] for col in v] for c, v in cols.items() if c != half})
        return self._finish(world, (cell, tag, wide, half))

    def _col(self, comp, k, m):
        kind, r = self.cols[comp][k], self.rng
        if kind == "f": return r.uniform(-100, 100, m).astype(F32).view(U32)
        if kind == "gen": return np.full(m, self.max_gen, dtype=U32)
        if kind == "u8": return r.integers(0, 2**8, m).astype(U8)
        if kind == "u16": return r.integers(0, 2**16, m).astype(U16)
        if kind == "u64": return r.integers(0, 2**64, m, dtype=U64)
        return r.integers(kind[0], kind[1], m).astype(U32)

    def extra_edit(self, x, A, B, ids):
        """Rekindle: fuses of 1 .. 3 for up to 64 cells, so that the next list spawns -- also behind lists that are still in flight."""
        r, n = self.rng, A.len
        if x >= 0.9 or not n: return None
        first = int(r.integers(0, n)); cnt = int(r.integers(1, min(n - first, 64) + 1))
        data = r.integers(1, 4, cnt).astype(U32)
        A.upload_word(ids[0], 2, first, data); B.upload_word(ids[0], 2, first, data)
        return f"rekindle [{first}:{first + cnt}]"

    def advance(self, frame, spawn): return bg.AdvanceFrame((int(self.rng.integers(0, 16)),))

    def spawns(self, q): return False                                           # (who spawns is decided on the device: the generator cannot know)


# ---- the committed seeds; the GPU tier and the CPU tier both read these ------------------------------------------------------------------------------------------
# chosen on the CPU (test_fuzz_device_spawn.py): every seed with n >= 64 meets every floor there; five smaller worlds (n = 1, 2, 63) ride along
SEEDS = (0, 6, 7, 8, 9, 14, 16, 17, 21, 22, 23, 31, 35, 37, 50, 53, 55, 57, 62, 68, 77, 84, 87, 88, 96)
TAGGED_SEEDS, SPEC_SEEDS = (0, 14, 57, 84), (9, 62, 87)
TILE = (6, 8150, 4)                                                             # (seed, n, n_lists): the children cross the 8192-slot layout tile


def run(seed, make_b, *, n=None, after_list=None, on_end=None, **kw):
    """fuzz_util.run of one committed seed with the FLAT adapter as backend A; returns (log, scenario, A's Counts)."""
    seen = {}

    def make_a(sc): seen["sc"] = sc; seen["A"] = sc.oracle(FLAT); return seen["A"]
    log = fuzz_util.run(seed, make_a, make_b, scenario=lambda s, big, max_n: ColonyScenario(s, n=n), after_list=after_list, on_end=on_end, **{**RUN_KW, **kw})
    return log, seen["sc"], seen["A"].counts


def cpu_pair(seed, **kw):
    """The generator guard: the FLAT adapter against the REFSHAPED one behind InFlight -- the stream the HIP backend gets."""
    rec = {}

    def make_b(sc): rec["B"] = InFlight(sc.oracle(REFSHAPED)); return rec["B"]

    def after_list(A, B, k, ctx): rec["alive"], rec["len"] = int(A.alive_mask(A.len).sum()), A.len
    log, sc, counts = run(seed, make_b, after_list=after_list, **kw)
    B = rec.pop("B")
    rec.update(log=log, n=sc.n, sc=sc, counts=counts, counts_b=B._w.counts, edited_in_flight=B.edited_in_flight, spawning_edited=B.spawning_edited)
    return rec
