"""Five features with special cases of their own on the host request path, as scenarios of the request fuzzer (fuzz_util.run(scenario=...)), and the oracle side of
each as ONE backend object (fuzz_user_worlds.OracleAdapter, generalised there).  Until this file each of them was tested on scripted SyncTest-shaped sessions (some
also as fan-out branch steps); none had met lists in any order, a frame loaded and advanced many times inside one list, a re-advance with other inputs, Saves that
evict their own source, host edits behind lists in flight, or the ring sweep.

    strategy   test_gpu_round5._f16_world (Accel: f32 x 3 Stored as 3 x f16; x exact, y lossy, z never written) + Count += input, and beside it
               Gen{value: u32, loads: u32} Stored as ONE u64 -- wider and fewer words than the component.  store packs both words, load unpacks them and sets
               loads + 1: not idempotent, all-integer, both words checksummed.  `loads` counts how often Strategy::load ran on the entity's lineage, so a Load that
               skipped ggrs_load because the row versions said "identical" ([Save(f), Load(f)]), or a Save that skipped ggrs_store, changes a checksum.  No system
               writes Gen: its columns change through Loads and host edits alone.
    inputs     branch_worlds_common.build_inputs: (input_bytes, players) from LAYOUTS, `const` drawn too; every AdvanceFrame carries drawn bytes, n_inputs in
               0 .. players (0 about once in sixteen), and in two thirds of the seeds a drawn InputStatus per player.
    bullets    test_gpu_round5._bullet_world: a user-written spawn system with a 16-byte payload record beside a user-written despawn, Kind outside the bundle.
               An `A*` AdvanceFrame carries FIRE and spawn_count / spawn_payload, a pure function of (seed, frame); Life is 2 .. 24, so entities die inside a session.
    hasher     test_gpu_schema.build_odd_hasher (a hasher no word list expresses) + Count-style `word 0 += input`.
    clock      resources_common.build_clock: rollback resources WITHOUT reduce or sum bindings -- the one world in which resources meet the lazy live block and
               deferred Saves.  ClockModel is kept beside the oracle and walked request by request, so that the entity callbacks' `pre` / `cur` view is right in a
               re-advance and behind a Load in the middle of a list; the host also writes Clock and Wind (resource_write), between lists and behind lists in flight.

What the scenarios keep away from, because the ORACLE cannot say what is right there (each is a limit of the model, not of the library):
  * float columns only ever get finite values (fuzz_user_worlds.py says why); Accel.y stays in [1, 2) times 1.001^frames, far below the f16 range.
  * Player only ever gets handles in 0 .. players: the device source indexes the input record with the handle after one `>=` test on an int -- a random u64
    would read outside the record.  BoxScenario has the same limit.
  * Gen.loads is written as 0 by the host (a new lineage), Gen.value as any u32.
Every scenario also takes `wrong=`: a deliberately WRONG restatement of its oracle side (WRONG below), which test_fuzz_feature_worlds.py uses as backend B to show
that the sessions would notice.  (A helper module, no tests of its own.)"""
import copy

import numpy as np

import bevy_ggrs_amd as bg
import branch_worlds_common as bw
import fuzz_user_worlds as fu
import fuzz_util
import resources_common as rc
import test_gpu_round5 as r5
import test_gpu_schema as sch
from oracle.binding import FLAT, REFSHAPED, OracleWorld

U8, U32, U64, F32 = np.uint8, np.uint32, np.uint64, np.float32
M32 = 0xFFFFFFFF
SIZES = fu.SIZES                                                  # (1, 2, 63, 64, 65, 257, 1025)
RUN_KW = {"n_lists": 20, "ring_sweep": True}
FAMILIES = ("strategy", "inputs", "bullets", "hasher", "clock")
WRONG = {"strategy": ("plain", "noload"), "inputs": ("status", "first_byte", "n_inputs"), "bullets": ("payload", "kind"), "hasher": ("builtin",),
         "clock": ("norestore", "stale_input")}

GEN_STRATEGY = """
__device__ void ggrs_store(const GgrsWords& t, GgrsWords& s) { s.u64(0) = (ggrs_u64)t.u32(0) | ((ggrs_u64)t.u32(1) << 32); }                  // Strategy::store
__device__ void ggrs_load(const GgrsWords& s, GgrsWords& t) { t.u32(0) = (ggrs_u32)s.u64(0); t.u32(1) = (ggrs_u32)(s.u64(0) >> 32) + 1u; }   // Strategy::load
"""


def gen_store(tg): return [(tg[0] & M32) | ((tg[1] & M32) << 32)]
def gen_load(sv): return [sv[0] & M32, ((sv[0] >> 32) + 1) & M32]
def gen_load_noload(sv): return [sv[0] & M32, (sv[0] >> 32) & M32]           # WRONG: leaves `loads` alone


# ---- the oracle side ---------------------------------------------------------------------------------------------------------------------------------------------
class FeatureAdapter(fu.OracleAdapter):
    """fuzz_user_worlds.OracleAdapter for worlds without begin_frame / land.  `passes`: frame -> the distinct (inputs, status, spawn_count) it was advanced with."""

    def __init__(self, oracle, model=None, stats=None, wrong=None, **more):
        super().__init__(oracle, model, stats if stats is not None else {}, hook=False, host_apply=False, wrong=wrong, passes={}, **more)

    def one(self, r):
        if not isinstance(r, bg.AdvanceFrame): return self.oracle.handle_requests([r])
        f = self.oracle.frame
        self.passes.setdefault(f, set()).add((tuple(x if isinstance(x, int) else bytes(x) for x in r.inputs), None if r.status is None else tuple(r.status), int(r.spawn_count)))
        return self.advance(r, f)

    def advance(self, r, frame): return self.oracle.handle_requests([r])

    def readvanced(self): return sum(len(s) > 1 for s in self.passes.values())


def shots(seed, frame, count=None):
    """The bullets of an `A*` AdvanceFrame: a PURE function of (seed, frame) -- a re-advanced frame that fires again fires the same shots."""
    if count is None: count = 1 + (frame * 7 + seed) % 5
    return count, np.random.default_rng([0xB011E7, seed, frame & M32]).uniform(-50, 50, (count, 4)).astype(F32)


class BulletAdapter(FeatureAdapter):
    """Counts per AdvanceFrame the children that came and the entities that went.  wrong="payload": every record is the one of frame - 1; wrong="kind": the children
    also get Kind, which their bundle does not carry."""

    def advance(self, r, frame):
        o, st = self.oracle, self.stats
        len0 = o.len
        alive0 = int(o.alive_mask(len0).sum()) if len0 else 0
        if self.wrong == "payload" and r.spawn_count:
            r = copy.copy(r); r.spawn_payload = shots(self.seed, frame - 1, r.spawn_count)[1]
        cs = o.handle_requests([r])
        built = o.len - len0
        st["children"] = st.get("children", 0) + built
        st["despawned"] = st.get("despawned", 0) + alive0 + built - (int(o.alive_mask(o.len).sum()) if o.len else 0)
        if self.wrong == "kind":
            for s in range(len0, o.len): o.insert_component(self.kind_id, s, np.zeros(1, dtype=U8))
        return cs

    def with_and_without(self): return sum(len({k[2] > 0 for k in s}) > 1 for s in self.passes.values())


class Clock(rc.ClockModel):
    """resources_common.ClockModel with the surface the adapter walks (begin / end / write) and one count: Loads that restored other words than the current ones.
    wrong="norestore": a Load leaves the resources alone; wrong="stale_input": every step takes the previous AdvanceFrame's input."""

    def __init__(self, wrong=None):
        super().__init__()
        self.wrong, self.restored_other, self.last_input = wrong, 0, 0

    def begin(self, inp0):
        self.step(self.last_input if self.wrong == "stale_input" else inp0)
        self.last_input = inp0

    def end(self): pass

    def load(self, frame):
        self.restored_other += self.snaps[frame] != self.cur
        if self.wrong == "norestore": self.pre = list(self.cur)
        else: super().load(frame)

    def write(self, res, words):
        """resource_write of the host: Clock = resource 0 (two words), Wind = 1, Big = 2."""
        if res == 0: self.cur[0], self.cur[1] = int(words[0]) & M32, int(words[1]) & M32
        else: self.cur[res + 1] = int(words[0])


class InFlight(fu.InFlight):
    """fuzz_user_worlds.InFlight, and how many resource writes found a list still in flight (res_in_flight)."""

    def __init__(self, w): super().__init__(w); self.__dict__["res_in_flight"] = 0

    def __getattr__(self, k):
        v = fu.InFlight.__getattr__(self, k)
        if k != "resource_write": return v

        def edit(*a, **kw):
            self.__dict__["res_in_flight"] += bool(self._q)
            return v(*a, **kw)
        return edit


# ---- the scenarios -----------------------------------------------------------------------------------------------------------------------------------------------
class _Feature(fu._UserScenario):
    """n from SIZES (or pinned), depth 1..8, capacity n + 128.  `cols` names what words() supplies per component word (_col)."""
    with_spawn, spawn_budget, adapter, ref_mode = False, 0, FeatureAdapter, REFSHAPED

    def __init__(self, seed, n=None):
        self._common(self.tag, seed, n)
        self._draw()

    def _draw(self): pass

    def describe(self): return f"{self.family} seed {self.seed}: n={self.n} depth={self.depth}{self._more()}"

    def _more(self): return ""

    def oracle(self, mode, wrong=None): return self.adapter(OracleWorld(self.capacity, 8, mode), wrong=wrong)

    def build(self, world):
        w = world.oracle if hasattr(world, "oracle") else world
        return self._finish(world, self._build(w, getattr(world, "wrong", None), world))

    def _col(self, comp, k, m):
        kind, r = self.cols[comp][k], self.rng
        if kind == "u32": return r.integers(0, 2**32, m, dtype=U64).astype(U32)
        if kind == "u8": return r.integers(0, 2**8, m).astype(U8)
        if kind == "zero": return np.zeros(m, dtype=U32)
        if kind == "handle": return r.integers(0, self.players + 1, m).astype(U64)
        if kind == "half": return (r.integers(-40, 41, m) * 0.5).astype(F32).view(U32)              # exact in f16
        if isinstance(kind[0], float): return r.uniform(kind[0], kind[1], m).astype(F32).view(U32)
        return r.integers(kind[0], kind[1], m).astype(U32)

    def spawns(self, q): return False

    def advance(self, frame, spawn): return bg.AdvanceFrame((int(self.rng.integers(0, 256)),))

    def extra_edit(self, x, A, B, ids):
        """One more upload of up to 64 slots of any word, so that these worlds see as many host edits -- behind lists in flight too -- as the worlds with a resource."""
        r, n = self.rng, A.len
        if x >= 0.92 or not n: return None
        c = int(r.integers(len(ids))); k = int(r.integers(len(self.cols[c])))
        first = int(r.integers(0, n)); cnt = int(r.integers(1, min(n - first, 64) + 1))
        data = self._col(c, k, cnt)
        A.upload_word(ids[c], k, first, data); B.upload_word(ids[c], k, first, data)
        return f"upload c{ids[c]}w{k}[{first}:{first + cnt}] (extra)"


class StrategyScenario(_Feature):
    """Two components under a Strategy in one world.  wrong="plain": the world built without its strategies; wrong="noload": Gen's load leaves `loads` alone."""
    family, tag = "strategy", 0x57A7
    ref_mode = FLAT                                                           # (the oracle keeps Strategies in its FLAT storage mode only: the CPU tier's pair is FLAT twice)
    #        Accel                                   Count     Gen {value, loads}
    cols = (("half", (1.0, 2.0), (-1000.0, 1000.0)), ("u32",), ("u32", "zero"))

    def _build(self, w, wrong, world):
        n, plain = self.n, wrong == "plain"
        A, C_ = r5._f16_world(w, not plain)
        bw._add_input(w, C_, 0)
        G = w.register_component("Gen", 4, 2)
        w.checksum_component(G, [0, 1])
        if not plain:
            if isinstance(w, OracleWorld): w.register_component_strategy(G, 8, 1, gen_store, gen_load_noload if wrong == "noload" else gen_load)
            else: w.register_component_strategy(G, 8, 1, GEN_STRATEGY)
        rng = np.random.default_rng(5)
        x = (rng.integers(-40, 40, n) * 0.5).astype(F32); y = rng.uniform(1, 2, n).astype(F32); z = rng.uniform(-1000, 1000, n).astype(F32)
        i = np.arange(n, dtype=U64)
        w.spawn(n, {A: [x.view(U32), y.view(U32), z.view(U32)], C_: [np.zeros(n, dtype=U32)], G: [((i * U64(2654435761)) & U64(M32)).astype(U32), np.zeros(n, dtype=U32)]})
        return A, C_, G

    def at_end(self, A):
        """The highest `loads` among the live entities that have Gen."""
        n = A.len
        if not n: return {"max_loads": 0}
        m = A.alive_mask(n) & A.present_mask(self.ids[2], n)
        return {"max_loads": int(np.where(m, A.download_word(self.ids[2], 1, 0, n), 0).max())}


class InputsScenario(_Feature):
    """wrong="status": a twin that sees every InputStatus as Confirmed; "first_byte": one that folds the first byte of an input and zeros for the rest; "n_inputs":
    one that takes n_inputs = players (the players without an input: zero bytes, Confirmed)."""
    family, tag = "inputs", 0x1EB07
    cols = (("u32",), ("handle",))

    def _draw(self):
        r = self.rng
        self.ib, self.players = bw.LAYOUTS[int(r.integers(len(bw.LAYOUTS)))]
        self.const = bool(r.random() < 0.125)
        self.with_status = bool(r.random() < 2 / 3)

    def _more(self): return f" input_bytes={self.ib} players={self.players} const={self.const} status={self.with_status}"

    def oracle(self, mode, wrong=None): return FeatureAdapter(OracleWorld(self.capacity, 8, mode), stats=bw.new_stats(), wrong=wrong)

    def _build(self, w, wrong, world):
        if wrong is None: return bw.build_inputs(w, self.n, self.ib, self.players, self.const, getattr(world, "stats", None))
        ib, players, right = self.ib, self.players, bw.input_twin(self.ib, self.const, world.stats)

        class View:
            def __init__(self, f): self.f = f; self.real = f.n_inputs; self.n_inputs = players if wrong == "n_inputs" else f.n_inputs; self.status = self
            def __getitem__(self, h): return 0 if wrong == "status" or h >= self.real else self.f.status[h]
            def input(self, h):
                b = self.f.input(h) if h < self.real else bytes(ib)
                return b[:1] + bytes(ib - 1) if wrong == "first_byte" else b
        orig, w.add_custom_system = w.add_custom_system, lambda fn, binds, **kw: orig(lambda words, slot, f: right(words, slot, View(f)), binds, **kw)
        try: return bw.build_inputs(w, self.n, ib, players, self.const, world.stats)
        finally: del w.add_custom_system

    def advance(self, frame, spawn):
        r = self.rng
        inp = r.integers(0, 256, size=(self.players, self.ib)).astype(U8)
        st = r.integers(0, 3, self.players)
        ni = int(r.integers(0, 16)); n_in = int(r.integers(1, self.players + 1))
        return bw.advance(inp, st if self.with_status else None, 0 if ni == 0 else n_in, self.ib)


class BulletsScenario(_Feature):
    family, tag, adapter = "bullets", 0xB011E7, BulletAdapter
    with_spawn, spawn_budget = True, 24                                       # at most 5 children each: 120 of the 128 spare slots
    LIFE = 5                                                                  # the spawner's iparam: a child lives 5 .. 9 frames
    #        Pos                              Vel                          Life       Kind
    cols = (((-50.0, 50.0), (-50.0, 50.0)), ((-5.0, 5.0), (-5.0, 5.0)), ((2, 25),), ("u8",))

    def oracle(self, mode, wrong=None): return BulletAdapter(OracleWorld(self.capacity, 8, mode), wrong=wrong, seed=self.seed, kind_id=3)

    def _build(self, w, wrong, world):
        n = self.n
        P, V, L, K = r5._bullet_world(w, life=self.LIFE)
        rng = np.random.default_rng(3)
        pos = rng.uniform(-10, 10, (n, 2)).astype(F32); vel = rng.uniform(-5, 5, (n, 2)).astype(F32)
        i = np.arange(n)
        w.spawn(n, {P: [pos[:, 0].copy().view(U32), pos[:, 1].copy().view(U32)], V: [vel[:, 0].copy().view(U32), vel[:, 1].copy().view(U32)], L: [(2 + i % 23).astype(U32)], K: [(i % 5).astype(U8)]})
        return P, V, L, K

    def advance(self, frame, spawn):
        r = self.rng
        a, b = int(r.integers(0, 16)), int(r.integers(0, 16))
        q = bg.AdvanceFrame(((a | r5.FIRE) if spawn else a, b))
        if spawn: q.spawn_count, q.spawn_payload = shots(self.seed, frame)
        return q

    def spawns(self, q): return bool(q.spawn_count)


class HasherScenario(_Feature):
    """wrong="builtin": the built-in word-list hash of the same four words in place of the user-written hasher."""
    family, tag = "hasher", 0x0DD
    cols = (("u32", "u32", "u32", "u32"),)

    def _build(self, w, wrong, world):
        extra = lambda w_, ids: bw._add_input(w_, ids[0], 0)      # noqa: E731
        if wrong is None: return sch.build_odd_hasher(w, self.n, extra=extra)
        orig, w.checksum_component_custom = w.checksum_component_custom, lambda comp, fn: w.checksum_component(comp, [0, 1, 2, 3])
        try: return sch.build_odd_hasher(w, self.n, extra=extra)
        finally: del w.checksum_component_custom


class ClockScenario(_Feature):
    """Fuses of 5 .. 64 frames: entities die mid-session.  Host edits of its own (extra_edit): resource_write of Clock (two u32) and of Wind (a finite float)."""
    family, tag = "clock", 0xC10C
    #        Pos               Seen              Fuse
    cols = (((-4.0, 4.0),), ("u32", "u32"), ((1, 65),))

    def oracle(self, mode, wrong=None): return FeatureAdapter(OracleWorld(self.capacity, 8, mode), model=Clock(wrong), wrong=wrong)

    def _build(self, w, wrong, world):
        ids = rc.build_clock(w, **({"model": world.model} if isinstance(w, OracleWorld) else {}))
        rc.spawn_clock(w, ids, self.n)
        return ids

    def advance(self, frame, spawn): return bg.AdvanceFrame((int(self.rng.integers(0, 16)),), dt_bits=rc.DT_BITS)

    def extra_edit(self, x, A, B, ids):
        r = self.rng
        if x < 0.84:
            words = [int(v) for v in r.integers(0, 2**32, 2, dtype=U64)]
            A.resource_write(0, words); B.resource_write(0, words)
            return f"Clock={words[0]:#x},{words[1]:#x}"
        bits = rc.f32_bits(F32(r.uniform(-8.0, 8.0)))
        A.resource_write(1, [bits]); B.resource_write(1, [bits])
        return f"Wind={bits:#x}"

    def extra_state(self, w):
        return {"resources": tuple(list(x) for x in (w.model.words() if hasattr(w, "model") else rc.read_resources(w)))}


SCENARIOS = {"strategy": StrategyScenario, "inputs": InputsScenario, "bullets": BulletsScenario, "hasher": HasherScenario, "clock": ClockScenario}

# ---- the committed seeds; the GPU tier and the CPU tier both read these -------------------------------------------------------------------------------------------
# chosen on the CPU among seeds 0 .. 159 (test_fuzz_feature_worlds.py holds them to its floors): per family the lowest fifteen seeds with n >= 64 that meet every
# event of the family and are told from every wrong restatement, three of each such size at least, and nine with n = 1, 2, 63.  Two of the floors are rare enough
# to decide the choice: a resource write behind a list in flight happens in about two clock seeds in five, and a third of the inputs seeds carries no InputStatus
# (sixteen of the twenty-four do; eight of the nine small ones do not).  Two of the inputs family's fifteen are 1-byte layouts, where the `first_byte` restatement
# is the right one and cannot be noticed.  TAGGED / DEFER / SPEC / FOLD are drawn from the default seeds, so that the CPU tier's guard over SEEDS covers every
# stream the GPU tier sees; DEFER holds seeds on which fuzz_util.deferral_model counts a deferring group and a read.
SEEDS = {"strategy": (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 19, 20, 23, 28, 32, 42),
         "inputs": (0, 3, 11, 12, 13, 14, 16, 19, 23, 24, 25, 26, 28, 31, 32, 34, 37, 39, 48, 56, 58, 60, 102, 108),
         "bullets": (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 19, 20, 21, 25, 26, 28, 37),
         "hasher": (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15, 23, 26, 28, 29, 30, 32, 33, 35, 62),
         "clock": (1, 3, 4, 5, 6, 7, 8, 9, 11, 12, 15, 22, 26, 28, 31, 33, 37, 40, 42, 44, 48, 58, 85, 101)}
DEFER = {"strategy": (1, 5, 8, 10, 11, 12, 13, 14), "inputs": (0, 3, 11, 12, 13, 14, 16, 19), "bullets": (0, 1, 2, 3, 4, 6, 7, 8), "hasher": (0, 1, 3, 6, 7, 8, 9, 13),
         "clock": (1, 4, 6, 9, 11, 12, 15, 26)}
_REST = {f: tuple(s for s in SEEDS[f] if s not in DEFER[f]) for f in FAMILIES}
TAGGED, SPEC, FOLD = ({f: _REST[f][a:b] for f in FAMILIES} for a, b in ((0, 8), (8, 12), (12, 16)))
# one pinned session per family across the 8192-slot layout tile: (seed, n, n_lists), with a branch-shaped list and a Load in the middle of a list
TILE = {"strategy": (0, 8262, 5), "inputs": (5, 8262, 5), "bullets": (12, 8262, 5), "hasher": (12, 8262, 5), "clock": (5, 8262, 5)}


def factory(family, n=None):
    return lambda seed, big, max_n: SCENARIOS[family](seed, n=n)


def run(family, seed, make_b, *, n=None, after_list=None, on_end=None, **kw):
    """fuzz_util.run of one committed case with the FLAT adapter as backend A; returns (log, scenario, A)."""
    seen = {}

    def make_a(sc): seen["sc"] = sc; seen["A"] = sc.oracle(FLAT); return seen["A"]

    def extra(w): return seen["sc"].extra_state(w) if hasattr(seen["sc"], "extra_state") else {}

    def end(A, B, log):
        if hasattr(seen["sc"], "at_end"): seen["end"] = seen["sc"].at_end(A)
        if on_end is not None: on_end(A, B, log)
    log = fuzz_util.run(seed, make_a, make_b, scenario=factory(family, n), extra_state=extra, after_list=after_list, on_end=end, **{**RUN_KW, **kw})
    seen["A"].__dict__["end"] = seen.get("end", {})
    return log, seen["sc"], seen["A"]


def cpu_pair(family, seed, wrong=None, **kw):
    """The generator guard: the FLAT adapter against the REFSHAPED one (sc.ref_mode) behind InFlight -- the stream the HIP backend gets.  wrong: backend B is that deliberately wrong
    restatement instead (the run then ought to raise).  Returns what the floors are counted from."""
    rec = {}

    def make_b(sc): rec["B"] = InFlight(sc.oracle(sc.ref_mode, wrong)); return rec["B"]
    log, sc, A = run(family, seed, make_b, **kw)
    B = rec.pop("B")
    rec.update(log=log, n=sc.n, sc=sc, A=A, stats=A.stats, end=A.end, edited_in_flight=B.edited_in_flight, res_in_flight=B.res_in_flight)
    return rec


def pairs(log):
    """(Loads directly followed by a Save, Saves of a frame f with a later Load of f in the same list), the ring sweep's lists left out."""
    ls = sl = 0
    for toks, is_sweep in fu._lists(log):
        if is_sweep: continue
        ls += sum(a[0] == "L" and b[0] == "S" for a, b in zip(toks, toks[1:]))
        saved = set()
        for t in toks:
            if t[0] == "S": saved.add(t[1:])
            elif t[0] == "L" and t[1:] in saved: sl += 1
    return ls, sl
