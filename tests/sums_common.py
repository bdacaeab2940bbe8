"""The worlds of the sum-binding tests (ggrs_hip_add_custom_system_sums: an entity system adds a float / double into a word of a device resource with e.sum_f32 /
e.sum_f64, and the frame's total is the BALANCED BINARY TREE OVER SLOT INDICES), each built twice: on a library world from HIP C++ source, and on the CPU oracle
(oracle.binding.OracleWorld, unchanged) from Python callbacks.

The oracle has no resources and gains none.  SumModel is a small Python restatement kept BESIDE it, after reduces_common.ReduceModel: the oracle's per-entity callbacks
are what says "the system ran for this entity" -- they add, typed and with one rounding per add, into the model's per-SLOT pending values (numpy float32 / float64,
-0.0 until somebody adds) --; end() computes the frame total with the tree literally as include/ggrs_hip.h defines it and adds it to the word with one add.
reduces_common.run_model drives it: the resource system in front of every AdvanceFrame, end() behind it, snapshots on SaveGameState, the resource checksum parts
XORed into the oracle's Checksum.  Everything is compared as BITS: resource words are unsigned ints on both sides.

    flock     components Pos{f32 x, f32 y}, Fuse{u32}; resources Centre{sx, sy: sums} (f32 x 2), Energy{e: sum, never reset} (f64), Census{alive: ADD} (u32)
                steer    (entity system, AHEAD of the summers)      Pos moves by 0.125 x (1 + (input & 3)) per axis toward last frame's Centre / 64
                reset    (resource system)                          sx = sy = 0; alive = 0                     -- the "sum per frame" idiom
                tally    (entity system)                            sums x into sx, y into sy, (double)x * x into e; reduces alive (+1)
                skew     (entity system, a SECOND summer of sx)     for slots with slot % 3 == 1: two more adds into sx -- per-slot order across systems and calls
                fuse     GGRS_SYS_SAT_SUB_DESPAWN on Fuse: entities die mid-session
              checksums: every component and every resource
    plain     the comparison world of scripts/bench_sums.py: the flock world with the e.sum_* calls (and the sum bindings) removed
    ureduce   ... with the sums replaced by u32 ADD reducers of the values' bits (the reduce-binding path: one atomic per wave)
(A helper module, no tests of its own.)"""
import numpy as np

import bevy_ggrs_amd as bg
import common as cm  # noqa: F401
from oracle.binding import OracleWorld
from oracle.oracle_np import SeaHasher
from reduces_common import combine, identity
from resources_common import DT_BITS  # noqa: F401

U32 = np.uint32
F32, F64 = np.float32, np.float64
SUM = "sum"
NEG_ZERO_32, NEG_ZERO_64 = 0x80000000, 0x8000000000000000


def f32_bits(v): return int(np.array([v], dtype=F32).view(np.uint32)[0])
def f64_bits(v): return int(np.array([v], dtype=F64).view(np.uint64)[0])
def bits_f32(b): return np.array([b & 0xFFFFFFFF], dtype=np.uint32).view(F32)[0]
def bits_f64(b): return np.array([b & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64).view(F64)[0]


def tree_sum(a):
    """The frame total T of include/ggrs_hip.h: pad the per-slot values to a power of two with -0.0, then x[2i] + x[2i+1] level by level until one value is left."""
    y = np.asarray(a)
    p = 1
    while p < max(1, len(y)): p *= 2
    y = np.concatenate([y, np.full(p - len(y), -0.0, dtype=y.dtype)])
    while len(y) > 1: y = y[0::2] + y[1::2]
    return y[0]


def seq_sum(a):
    """a[0] + a[1] + .. in slot order, one rounding per add, starting from -0.0."""
    t = a.dtype.type(-0.0)
    for v in a: t = t + v
    return t


def other_orders(a):
    """The three orders an implementation that is NOT the tree would most likely produce: slot order, reverse slot order, sequential per 64 then sequential."""
    per64 = np.array([seq_sum(a[i:i + 64]) for i in range(0, len(a), 64)], dtype=a.dtype)
    return seq_sum(a), seq_sum(a[::-1]), seq_sum(per64)


def bits_of(v):
    return f64_bits(v) if np.asarray(v).dtype == F64 else f32_bits(v)


class SumModel:
    """The resources of a world beside the oracle.  layout = [(resource, word bytes, [(init bits, None | SUM | GGRS_EFFECT_* op), ..])].  cur: the words' bits as the
    last frame left them; pre: cur before this frame's resource system ran; pend: per summed word one value per slot (-0.0), per reduced word the op's running value."""

    def __init__(self, layout, n_slots, resource_system=None):
        self.layout, self.n_slots = layout, n_slots
        self.cur = [[init for init, _ in words] for _, _, words in layout]
        self.pre = [list(r) for r in self.cur]
        self.resource_system = resource_system
        self.snaps = {}
        self.sent = 0
        self._clear()

    def _clear(self):
        self.pend = [[None if kind is None else (np.full(self.n_slots, -0.0, dtype=F64 if wb == 8 else F32) if kind == SUM else identity(kind, wb)) for _, kind in words]
                     for _, wb, words in self.layout]

    def sum(self, r, k, slot, v):
        """e.sum_f32 / e.sum_f64 for the entity at `slot`: a_s = a_s + v in the word's type, one rounding."""
        p = self.pend[r][k]
        p[slot] = p[slot] + p.dtype.type(v)
        self.sent += 1

    def reduce(self, r, k, v):
        _, wb, words = self.layout[r]
        self.pend[r][k] = combine(words[k][1], wb, self.pend[r][k], v)

    def begin(self, inp0):
        self.pre = [list(r) for r in self.cur]
        if self.resource_system: self.resource_system(self.cur, inp0)

    def end(self):
        """Behind an AdvanceFrame: every summed word becomes w + T, ONE add; every reduced word op(w, pending)."""
        for r, (_, wb, words) in enumerate(self.layout):
            for k, (_, kind) in enumerate(words):
                if kind == SUM:
                    T = tree_sum(self.pend[r][k])
                    self.cur[r][k] = f64_bits(bits_f64(self.cur[r][k]) + T) if wb == 8 else f32_bits(bits_f32(self.cur[r][k]) + T)
                elif kind is not None: self.cur[r][k] = combine(kind, wb, self.cur[r][k], self.pend[r][k])
        self._clear()

    def save(self, frame): self.snaps[frame] = [list(r) for r in self.cur]

    def load(self, frame): self.cur = [list(r) for r in self.snaps[frame]]; self.pre = [list(r) for r in self.cur]

    def part(self, state=None):
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


def read_resources(w, n=3):
    return tuple(w.resource_read(r) for r in range(n))


# ---- initial values under which the ORDER of a float sum shows --------------------------------------------------------------------------------------------------
def order_values(n, shift=0):
    """v_i = f32(200 + (37 i) mod 211) x f32(0.37) x 2^((5 i) mod 7 - 3), negated where (3 i) & 4: mixed magnitudes and signs, so that the balanced tree, the slot-order
    sum, the reverse-order sum and sequential-per-64-then-sequential all round differently (test_sums_text.py asserts it for the sizes the GPU tests use)."""
    i = np.arange(shift, shift + n, dtype=np.int64)
    v = (200 + (37 * i) % 211).astype(F32) * F32(0.37) * np.exp2(((5 * i) % 7 - 3).astype(F32)).astype(F32)
    return np.where((3 * i) & 4, -v, v).astype(F32)


# ---- flock ------------------------------------------------------------------------------------------------------------------------------------------------------
ENERGY_INIT = f64_bits(0.5)
FLOCK_LAYOUT = [("Centre", 4, [(0, SUM), (0, SUM)]), ("Energy", 8, [(ENERGY_INIT, SUM)]), ("Census", 4, [(0, bg.EFFECT_ADD)])]
STEER_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const float step = 0.125f * (float)(1 + (f.input[0] & 3));
    const float cx = e.res_f32(0) * 0.015625f, cy = e.res_f32(1) * 0.015625f;
    e.f32(0) = e.f32(0) + (cx > e.f32(0) ? step : -step);
    e.f32(1) = e.f32(1) + (cy > e.f32(1) ? step : -step);
}
"""
RESET_SRC = "__device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame&) { r.f32(0) = 0.f; r.f32(1) = 0.f; r.u32(2) = 0u; }"
TALLY_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) {
    e.sum_f32(0, e.f32(0)); e.sum_f32(1, e.f32(1)); e.sum_f64(2, (double)e.f32(0) * (double)e.f32(0)); e.reduce_u32(0, 1u);
}
"""
SKEW_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) {
    if (e.slot % 3u == 1u) { e.sum_f32(0, e.f32(1) * 0.5f); e.sum_f32(0, e.f32(0) * -0.25f); }
}
"""
TALLY_PLAIN_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.reduce_u32(0, 1u); }"
SKEW_PLAIN_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.f32(0) = e.f32(0); }"
TALLY_UREDUCE_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) {
    e.reduce_u32(1, e.u32(0)); e.reduce_u32(2, e.u32(1)); e.reduce_u32(3, e.u32(0) * 3u); e.reduce_u32(0, 1u);
}
"""
SKEW_UREDUCE_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) {
    if (e.slot % 3u == 1u) { e.reduce_u32(0, e.u32(1) >> 1); e.reduce_u32(0, e.u32(0) >> 2); }
}
"""


def flock_reset(cur, inp0):
    cur[0][0] = 0; cur[0][1] = 0; cur[2][0] = 0


def flock_model(n_slots):
    return SumModel(FLOCK_LAYOUT, n_slots, flock_reset)


def build_flock(w, *, model=None, variant="sums", fuse_step=1):
    """Registers the flock world on `w` (a library world, or the oracle with its SumModel); returns (Pos, Fuse).  variant (a library world only): "sums", or the
    comparison worlds "plain" and "ureduce"."""
    Pos = w.register_component("Pos", 4, 2); Fz = w.register_component("Fuse", 4, 1)
    w.checksum_component(Pos, [0, 1]); w.checksum_component(Fz, [0])
    if isinstance(w, OracleWorld):
        def steer(words, slot, f):
            step = F32(0.125) * F32(1 + (f.input(0)[0] & 3))
            cx, cy = bits_f32(model.pre[0][0]) * F32(0.015625), bits_f32(model.pre[0][1]) * F32(0.015625)
            x, y = bits_f32(words[0]), bits_f32(words[1])
            return [f32_bits(x + (step if cx > x else -step)), f32_bits(y + (step if cy > y else -step))], 0

        def tally(words, slot, f):
            x, y = bits_f32(words[0]), bits_f32(words[1])
            model.sum(0, 0, slot, x); model.sum(0, 1, slot, y); model.sum(1, 0, slot, F64(x) * F64(x)); model.reduce(2, 0, 1)
            return list(words), 0

        def skew(words, slot, f):
            x, y = bits_f32(words[0]), bits_f32(words[1])
            if slot % 3 == 1: model.sum(0, 0, slot, y * F32(0.5)); model.sum(0, 0, slot, x * F32(-0.25))
            return list(words), 0
        for fn in (steer, tally, skew): w.add_custom_system(fn, [(Pos, 0), (Pos, 1)])
    else:
        Ce, En, Cn = register_model_resources(w, flock_model(1))
        w.add_custom_system(STEER_SRC, [(Pos, 0), (Pos, 1)], name="steer", resources=[(Ce, 0), (Ce, 1)])
        w.add_resource_system(RESET_SRC, [(Ce, 0), (Ce, 1), (Cn, 0)], name="reset")
        if variant == "sums":
            w.add_custom_system(TALLY_SRC, [(Pos, 0), (Pos, 1)], name="tally", reduces=[(Cn, 0, bg.EFFECT_ADD)], sums=[(Ce, 0), (Ce, 1), (En, 0)])
            w.add_custom_system(SKEW_SRC, [(Pos, 0), (Pos, 1)], name="skew", sums=[(Ce, 0)])
        elif variant == "plain":
            w.add_custom_system(TALLY_PLAIN_SRC, [(Pos, 0), (Pos, 1)], name="tally", reduces=[(Cn, 0, bg.EFFECT_ADD)])
            w.add_custom_system(SKEW_PLAIN_SRC, [(Pos, 0), (Pos, 1)], name="skew")
        else:
            Ux = w.register_resource("Bits", 4, 3, [0, 0, 0]); w.checksum_resource(Ux, [0, 1, 2])
            w.add_custom_system(TALLY_UREDUCE_SRC, [(Pos, 0), (Pos, 1)], name="tally",
                                reduces=[(Cn, 0, bg.EFFECT_ADD), (Ux, 0, bg.EFFECT_ADD), (Ux, 1, bg.EFFECT_ADD), (Ux, 2, bg.EFFECT_ADD)])
            w.add_custom_system(SKEW_UREDUCE_SRC, [(Pos, 0), (Pos, 1)], name="skew", reduces=[(Ux, 0, bg.EFFECT_ADD)])
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(Fz,), word=(0,), iparam=(fuse_step, bg.DESPAWN_IMMEDIATE))
    return Pos, Fz


def flock_xy(first, m):
    return order_values(m, first), order_values(m, first + 17) * F32(0.75)


def spawn_flock(w, ids, n, *, filler=0, tail=0, fuse_base=5, fuse_mod=60):
    """n flock entities; then `filler` entities that have Fuse alone (no user-written system visits them: the oracle stays cheap, the launch covers them, their slots
    keep -0.0) and `tail` flock entities behind those -- in the last workgroups of a large grid."""
    Pos, Fz = ids

    def full(first, m):
        i = np.arange(first, first + m)
        x, y = flock_xy(first, m)
        w.spawn(m, {Pos: [x.view(U32), y.view(U32)], Fz: [(fuse_base + (i * 7) % fuse_mod).astype(U32)]})
    full(0, n)
    if filler: w.spawn(filler, {Fz: [np.full(filler, 1 << 20, dtype=U32)]})
    if tail: full(n + filler, tail)


def sum_partials(w, word, n_units):
    """The 8-byte partial entries of summed word `word` for units [0, n_units), as uint64 (ggrs_dbg_sum_partials)."""
    import ctypes as C
    buf = (C.c_uint64 * n_units)()
    w._lib.ggrs_dbg_sum_partials.restype = C.c_int64
    w._lib.ggrs_dbg_sum_partials.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
    got = w._lib.ggrs_dbg_sum_partials(w._p, word, buf, 8 * n_units)
    assert got >= 8 * n_units, got
    return np.array(buf, dtype=np.uint64)
