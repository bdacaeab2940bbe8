"""The worlds of the reduce-binding tests (ggrs_hip_add_custom_system_reduces: an entity system combines a value into a word of a device resource with e.reduce_*),
each built twice: on a library world from HIP C++ source, and on the CPU oracle (oracle.binding.OracleWorld, unchanged) from Python callbacks.

The oracle has no resources and gains none.  ReduceModel (CensusModel: the census world's) is a small Python restatement kept BESIDE it, after resources_common.ClockModel: the oracle's per-entity
callbacks are what says "the system ran for this entity" -- they combine into the model's PENDING values --; run_model runs the world's resource system in front of
every AdvanceFrame and applies the pending values after it (all reductions of a frame land at the end of the frame), snapshots on SaveGameState, restores on
LoadGameState, and XORs the resource checksum parts (oracle.oracle_np.SeaHasher) into the oracle's Checksum.

    census    components Hp{u32}, Seen{u32}, Fuse{u32}; resources Census{alive: ADD, flags: OR} (u32 x 2), Low{hp: MIN_U} (u32), Total{hp_sum: ADD} (u64, never reset)
                look     (entity system, AHEAD of the reducers)    Seen = Census.alive                      -- last frame's result, fed back into checksummed state
                reset    (resource system)                          alive = 0; flags = input << 16; hp = 0xFFFFFFFF     -- the "count per frame" idiom
                wound    (entity system)                            Hp drops by 1 + ((input + slot) & 3); reduces flags only when (Hp & 7) == 3
                count    (entity system)                            reduces alive (+1), hp (min Hp), hp_sum (+ Hp x 0x100000001)
                fuse     GGRS_SYS_SAT_SUB_DESPAWN on Fuse: entities die mid-session
              checksums: every component and every resource
    plain     the comparison world of scripts/bench_reduces.py: the census world with the reduce_* calls (and the reduce bindings) removed
    ops       one component Val{u32}; one resource of eight words of one width, word k under op k; `mix` (a resource system) puts the identities back on odd inputs;
              `feed` (entity system) steps Val by an LCG and reduces it into all eight words: values of both signs, an ADD that wraps
    big       one 4-byte component under GGRS_SYS_ADD_U32 that every entity has, the census components that only a few have, `reset` and `count`: the in-place test
(A helper module, no tests of its own.)"""
import numpy as np

import bevy_ggrs_amd as bg
import common as cm
from oracle.binding import OracleWorld
from oracle.oracle_np import SeaHasher
from resources_common import DT_BITS, _Recorder, stamp

U32 = np.uint32
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
OPS = (bg.EFFECT_ADD, bg.EFFECT_MIN_U, bg.EFFECT_MAX_U, bg.EFFECT_MIN_I, bg.EFFECT_MAX_I, bg.EFFECT_OR, bg.EFFECT_AND, bg.EFFECT_XOR)
TOTAL_INIT = 1 << 40


def identity(op, wb):
    ones = M64 if wb == 8 else M32
    return {bg.EFFECT_MIN_U: ones, bg.EFFECT_AND: ones, bg.EFFECT_MIN_I: ones >> 1, bg.EFFECT_MAX_I: (ones >> 1) + 1}.get(op, 0)


def combine(op, wb, x, v):
    """x op v on words of wb bytes, as kernels.hpp fx_combine: wrapping add, unsigned / signed min and max, or, and, xor."""
    ones = M64 if wb == 8 else M32
    x &= ones; v &= ones
    sgn = lambda a: a - (ones + 1) if a >> (8 * wb - 1) else a      # noqa: E731
    if op == bg.EFFECT_ADD: return (x + v) & ones
    if op == bg.EFFECT_MIN_U: return min(x, v)
    if op == bg.EFFECT_MAX_U: return max(x, v)
    if op == bg.EFFECT_MIN_I: return v if sgn(v) < sgn(x) else x
    if op == bg.EFFECT_MAX_I: return v if sgn(v) > sgn(x) else x
    if op == bg.EFFECT_OR: return x | v
    if op == bg.EFFECT_AND: return x & v
    return x ^ v


class ReduceModel:
    """The resources of a world beside the oracle.  layout = [(resource, word bytes, [(init, op or None), ..])]: a word with an op is reduced into.  cur: the values as
    the last frame left them; pre: cur before this frame's resource system ran; pend: what the entity callbacks sent in the frame being simulated."""

    def __init__(self, layout, resource_system=None):
        self.layout = layout
        self.cur = [[init for init, _ in words] for _, _, words in layout]
        self.pre = [list(r) for r in self.cur]
        self.resource_system = resource_system
        self.snaps = {}
        self.sent = 0
        self._clear()

    def _clear(self):
        self.pend = [[None if op is None else identity(op, wb) for _, op in words] for _, wb, words in self.layout]

    def reduce(self, r, k, v):
        _, wb, words = self.layout[r]
        self.pend[r][k] = combine(words[k][1], wb, self.pend[r][k], v)
        self.sent += 1

    def begin(self, inp0):
        """In front of an AdvanceFrame: the resource system, which in these worlds is registered behind the readers (`pre`) and ahead of the reducers."""
        self.pre = [list(r) for r in self.cur]
        if self.resource_system: self.resource_system(self.cur, inp0)

    def end(self):
        """Behind it: the frame's reductions land."""
        for r, (_, wb, words) in enumerate(self.layout):
            for k, (_, op) in enumerate(words):
                if op is not None: self.cur[r][k] = combine(op, wb, self.cur[r][k], self.pend[r][k])
        self._clear()

    def save(self, frame): self.snaps[frame] = [list(r) for r in self.cur]

    def load(self, frame): self.cur = [list(r) for r in self.snaps[frame]]; self.pre = [list(r) for r in self.cur]

    def part(self, state=None):
        """The XOR of the ChecksumParts (resource_checksum.rs:63-83): checksum_hasher() fed each resource's words in order, each with its own width."""
        s = self.cur if state is None else state
        x = 0
        for r, (_, wb, words) in enumerate(self.layout):
            h = SeaHasher()
            for k in range(len(words)): h.write(int(s[r][k]).to_bytes(wb, "little"))
            x ^= h.finish()
        return x

    def words(self, state=None):
        s = self.cur if state is None else state
        return tuple(list(r) for r in s)


def register_model_resources(w, model):
    ids = []
    for name, wb, words in model.layout:
        r = w.register_resource(name, wb, len(words), [init for init, _ in words]); w.checksum_resource(r, list(range(len(words)))); ids.append(r)
    return ids


# ---- census ---------------------------------------------------------------------------------------------------------------------------------------------------
CENSUS_LAYOUT = [("Census", 4, [(0, bg.EFFECT_ADD), (0, bg.EFFECT_OR)]), ("Low", 4, [(M32, bg.EFFECT_MIN_U)]), ("Total", 8, [(TOTAL_INIT, bg.EFFECT_ADD)])]
LOOK_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) = e.res_u32(0); }"
RESET_SRC = r"""
__device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame& f) {
    r.u32(0) = 0u; r.u32(1) = (ggrs_u32)f.input[0] << 16; r.u32(2) = 0xFFFFFFFFu;
}
"""
WOUND_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u32 d = 1u + (((ggrs_u32)f.input[0] + (ggrs_u32)e.slot) & 3u);
    e.u32(0) = e.u32(0) > d ? e.u32(0) - d : 0u;
    if ((e.u32(0) & 7u) == 3u) e.reduce_u32(0, 1u << ((ggrs_u32)e.slot & 15u));
}
"""
WOUND_PLAIN_SRC = WOUND_SRC.replace("    if ((e.u32(0) & 7u) == 3u) e.reduce_u32(0, 1u << ((ggrs_u32)e.slot & 15u));\n", "")
COUNT_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) {
    e.reduce_u32(0, 1u); e.reduce_u32(1, e.u32(0)); e.reduce_u64(2, (ggrs_u64)e.u32(0) * 0x100000001ull);
}
"""
COUNT_PLAIN_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) = e.u32(0); }"


def census_reset(cur, inp0):
    cur[0][0] = 0; cur[0][1] = ((inp0 & 0xFF) << 16) & M32; cur[1][0] = M32


class CensusModel(ReduceModel):
    """Census{alive, flags}, Low{hp}, Total{hp_sum} beside the oracle, with `reset` as the frame's resource system."""

    def __init__(self): super().__init__(CENSUS_LAYOUT, census_reset)


def census_model():
    return CensusModel()


def add_census_reducers(w, res, Hp, *, with_wound=True):
    Cn, Lo, To = res
    if with_wound: w.add_custom_system(WOUND_SRC, [(Hp, 0)], name="wound", reduces=[(Cn, 1, bg.EFFECT_OR)])
    w.add_custom_system(COUNT_SRC, [(Hp, 0)], name="count", reduces=[(Cn, 0, bg.EFFECT_ADD), (Lo, 0, bg.EFFECT_MIN_U), (To, 0, bg.EFFECT_ADD)])


def build_census(w, *, model=None, plain=False, fuse_step=1):
    """Registers the census world on `w` (a library world, or the oracle with its ReduceModel); returns (Hp, Seen, Fuse).  plain: the comparison world -- the same
    resources and systems with the reduce_* calls and the reduce bindings removed (a library world only)."""
    Hp = w.register_component("Hp", 4, 1); Sn = w.register_component("Seen", 4, 1); Fz = w.register_component("Fuse", 4, 1)
    for c in (Hp, Sn, Fz): w.checksum_component(c, [0])
    if isinstance(w, OracleWorld):
        def look(words, slot, f): return [model.pre[0][0]], 0

        def wound(words, slot, f):
            d = 1 + ((f.input(0)[0] + slot) & 3)
            hp = words[0] - d if words[0] > d else 0
            if (hp & 7) == 3: model.reduce(0, 1, 1 << (slot & 15))
            return [hp], 0

        def count(words, slot, f):
            model.reduce(0, 0, 1); model.reduce(1, 0, words[0]); model.reduce(2, 0, words[0] * 0x100000001)
            return [words[0]], 0
        w.add_custom_system(look, [(Sn, 0)]); w.add_custom_system(wound, [(Hp, 0)]); w.add_custom_system(count, [(Hp, 0)])
    else:
        res = register_model_resources(w, census_model())
        Cn, Lo, To = res
        w.add_custom_system(LOOK_SRC, [(Sn, 0)], name="look", resources=[(Cn, 0)])
        w.add_resource_system(RESET_SRC, [(Cn, 0), (Cn, 1), (Lo, 0)], name="reset")
        if plain:
            w.add_custom_system(WOUND_PLAIN_SRC, [(Hp, 0)], name="wound"); w.add_custom_system(COUNT_PLAIN_SRC, [(Hp, 0)], name="count")
        else: add_census_reducers(w, res, Hp)
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(Fz,), word=(0,), iparam=(fuse_step, bg.DESPAWN_IMMEDIATE))
    return Hp, Sn, Fz


def spawn_census(w, ids, n, *, filler=0, tail=0, fuse_base=5, fuse_mod=60):
    """n census entities; then `filler` entities that have Fuse alone (no user-written system visits them: the oracle stays cheap, the launch covers them) and `tail`
    census entities behind those -- in the last workgroups of a large grid."""
    Hp, Sn, Fz = ids

    def full(first, m):
        i = np.arange(first, first + m)
        w.spawn(m, {Hp: [(200 + (i * 37) % 211).astype(U32)], Sn: [np.zeros(m, dtype=U32)], Fz: [(fuse_base + (i * 7) % fuse_mod).astype(U32)]})
    full(0, n)
    if filler: w.spawn(filler, {Fz: [np.full(filler, 1 << 20, dtype=U32)]})
    if tail: full(n + filler, tail)


# ---- ops: all eight ops on words of one width -----------------------------------------------------------------------------------------------------------------
def ops_layout(wb):
    return [("Acc", wb, [(identity(op, wb), op) for op in OPS])]


def ops_mix(wb):
    def mix(cur, inp0):
        if inp0 & 1: cur[0][:] = [identity(op, wb) for op in OPS]
    return mix


def _mix_src(wb):
    lit = (lambda v: f"0x{v:x}ull") if wb == 8 else (lambda v: f"0x{v:x}u")
    acc = "u64" if wb == 8 else "u32"
    body = " ".join(f"r.{acc}({k}) = {lit(identity(op, wb))};" for k, op in enumerate(OPS))
    return "__device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame& f) { if (f.input[0] & 1) { %s } }" % body


def _feed_value(v, wb):
    return v if wb == 4 else ((v << 32) | ((v * 2654435761) & M32))


def _feed_src(wb):
    val = "v" if wb == 4 else "(((ggrs_u64)v << 32) | (ggrs_u64)(ggrs_u32)(v * 2654435761u))"
    calls = " ".join(f"e.reduce_{'u64' if wb == 8 else ('i32' if op in (bg.EFFECT_MIN_I, bg.EFFECT_MAX_I) else 'u32')}({k}, {'(int)' if wb == 4 and op in (bg.EFFECT_MIN_I, bg.EFFECT_MAX_I) else ''}{val});"
                     for k, op in enumerate(OPS))
    # an accessor of the other width does nothing (binding 0 is the ADD word): the model never sees these calls
    other = "e.reduce_u64(0, 5ull);" if wb == 4 else "e.reduce_u32(0, 5u); e.reduce_i32(0, -5);"
    return ("__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) { const ggrs_u32 v = e.u32(0) * 1664525u + 1013904223u + (ggrs_u32)f.input[0]; e.u32(0) = v; %s %s }"
            % (calls, other))


def build_ops(w, wb, *, model=None):
    V = w.register_component("Val", 4, 1); w.checksum_component(V, [0])
    if isinstance(w, OracleWorld):
        def feed(words, slot, f):
            v = (words[0] * 1664525 + 1013904223 + f.input(0)[0]) & M32
            for k in range(len(OPS)): model.reduce(0, k, _feed_value(v, wb))
            return [v], 0
        w.add_custom_system(feed, [(V, 0)])
    else:
        (A,) = register_model_resources(w, ReduceModel(ops_layout(wb)))
        w.add_resource_system(_mix_src(wb), [(A, k) for k in range(len(OPS))], name="mix")
        w.add_custom_system(_feed_src(wb), [(V, 0)], name="feed", reduces=[(A, k, op) for k, op in enumerate(OPS)])
    return (V,)


# ---- big: the in-place world ----------------------------------------------------------------------------------------------------------------------------------
def build_big(w, *, model=None):
    """Every entity has Acc (GGRS_SYS_ADD_U32: built-in on both sides); the few census entities also have Hp, which `count` reduces."""
    A = w.register_component("Acc", 4, 1); Hp = w.register_component("Hp", 4, 1)
    w.checksum_component(A, [0]); w.checksum_component(Hp, [0])
    w.add_system(bg.SYS_ADD_U32, comp=(A,), word=(0,), iparam=(3,))
    if isinstance(w, OracleWorld):
        def count(words, slot, f):
            model.reduce(0, 0, 1); model.reduce(1, 0, words[0]); model.reduce(2, 0, words[0] * 0x100000001)
            return [words[0]], 0
        w.add_custom_system(count, [(Hp, 0)])
    else:
        res = register_model_resources(w, census_model())
        Cn, Lo, To = res
        w.add_resource_system(RESET_SRC, [(Cn, 0), (Cn, 1), (Lo, 0)], name="reset")
        add_census_reducers(w, res, Hp, with_wound=False)
    return A, Hp


# ---- request lists and the walk of oracle + model ------------------------------------------------------------------------------------------------------------------
def synctest_lists(cd, ticks, depth=8):
    from peer_effects_common import synctest_lists as sl
    return stamp(sl(cd, ticks, depth=depth, inputs=lambda t: ((t * 5 + 3) & 15,)))


def p2p_lists(ticks, max_rollback=8, seed=4):
    """P2P-shaped rollbacks of 0 .. max_rollback - 1 frames whose inputs CHANGE between prediction and confirmation (as resources_common.p2p_lists)."""
    rec = _Recorder()
    drv = cm.P2PShapeDriver(rec, max_rollback=max_rollback, seed=seed, inputs=lambda frame: ((frame * 7 + 3 * len(drv.depths)) & 15,))
    for _ in range(ticks): drv.tick()
    stamp([reqs for _, reqs in rec.lists])
    return rec.lists


def run_model(o, model, reqs, *, cd=-1, confirmed=None, got=None):
    """One request list on the oracle AND the model, request by request; appends (frame, oracle checksum ^ resource parts) per Save to `got` and returns it."""
    got = [] if got is None else got
    if confirmed is not None: o.set_confirmed(confirmed)
    for r in reqs:
        if cd >= 0 and o.frame - cd >= 0: o.set_confirmed(o.frame - cd)
        if isinstance(r, bg.SaveGameState): model.save(r.frame)
        elif isinstance(r, bg.LoadGameState): model.load(r.frame)
        else: model.begin(int(r.inputs[0]) if len(r.inputs) else 0)
        cs = o.handle_requests([r])
        if isinstance(r, bg.AdvanceFrame): model.end()
        if isinstance(r, bg.SaveGameState): got.append((r.frame, cs[0] ^ model.part()))
    return got


def read_resources(w, n=3):
    return tuple(w.resource_read(r) for r in range(n))


def inbox_is_identities(w, layout):
    """The reduce inbox as the last host call left it: every reduced word of every line at its op's identity."""
    import ctypes as C
    buf = (C.c_uint8 * 4096)()
    w._lib.ggrs_dbg_reduce_inbox.restype = C.c_int64
    w._lib.ggrs_dbg_reduce_inbox.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    n = w._lib.ggrs_dbg_reduce_inbox(w._p, buf, 4096)
    assert n > 0 and n % 64 == 0, n
    raw = bytes(buf)[:n]
    # a cell holds the 8-byte resources first, then the 4-byte ones, each in registration order
    off, at = 0, {}
    for wb_pass in (8, 4):
        for r, (_, wb, words) in enumerate(layout):
            if wb == wb_pass: at[r] = off; off += wb * len(words)
    for line in range(n // 64):
        for r, (_, wb, words) in enumerate(layout):
            for k, (_, op) in enumerate(words):
                if op is None: continue
                o_ = line * 64 + at[r] + k * wb
                if int.from_bytes(raw[o_:o_ + wb], "little") != identity(op, wb): return False
    return True
