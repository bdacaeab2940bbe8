"""The worlds of the device-resource tests (ggrs_hip_register_resource / _add_resource_system / _add_custom_system_resources), each built twice: on a library world
from HIP C++ source, and on the CPU oracle (oracle.binding.OracleWorld, unchanged) from Python callbacks.

The oracle has no resources and gains none.  ClockModel is a small Python restatement of the resource chain kept BESIDE it: it steps on every AdvanceFrame of the
same request list with that request's inputs, snapshots on SaveGameState, restores on LoadGameState, and shows the oracle's entity callbacks the values "as of
system position i" (`pre`: before the resource system ran in the frame being simulated, `cur`: after).  The expected Checksum is the oracle's XOR the resource parts
computed with oracle.oracle_np.SeaHasher -- all the reference's XOR fold requires (checksum.rs:94).

    clock     components Pos{x: f32}, Seen{before: u32, after: u32}, Fuse{u32}; resources Clock{ticks, seed: u32}, Wind{x: f32}, Big{acc: u64}
                before   (entity system, registered AHEAD of tick)   Seen.before = Clock.ticks            -- the OLD value
                tick     (resource system)                            ticks += 1; seed = LCG(seed) ^ input; Wind.x = f(seed, dt); acc += 0x100000001 * seed
                drift    (entity system, registered AFTER tick)      Pos.x += Wind.x * dt; Seen.after = Clock.ticks   -- the NEW value
                fuse     GGRS_SYS_SAT_SUB_DESPAWN on Fuse: entities die mid-session
              checksums: every component, Clock (both words), Wind, Big
    plain     the comparison world of the launch-count test and scripts/bench_resources.py: the clock world with `tick` removed and `drift` reading constants
    big       one 4-byte component, built-in systems only (GGRS_SYS_ADD_U32) on the oracle side, the same resources and `tick`: the in-place test at 1 M slots
(A helper module, no tests of its own.)"""
import numpy as np

import bevy_ggrs_amd as bg
import common as cm
from oracle.binding import OracleWorld
from oracle.oracle_np import SeaHasher

F32, U32, U64 = np.float32, np.uint32, np.uint64
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
DT = F32(1.0) / F32(60.0)
DT_BITS = int(np.array([DT], dtype=F32).view(U32)[0])
WIND_SCALE, WIND_BIAS = F32(2.0 ** -20), F32(3.0)           # the resource system's fparam[0], fparam[1]
CLOCK_INIT, WIND_INIT, BIG_INIT = (0, 12345), 0.0, 1 << 40

# bindings: 0 = Clock.ticks, 1 = Clock.seed, 2 = Wind.x, 3 = Big.acc
TICK_SRC = r"""
__device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame& f) {
    r.u32(0) += 1u;
    r.u32(1) = (r.u32(1) * 1664525u + 1013904223u) ^ (ggrs_u32)f.input[0];
    r.f32(2) = (float)(r.u32(1) >> 8) * f.fparam[0] + f.dt * f.fparam[1];
    r.u64(3) += 0x100000001ull * (ggrs_u64)r.u32(1);
}
"""
# binding 0 = Seen.before; resource binding 0 = Clock.ticks
BEFORE_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) = e.res_u32(0); }"
# bindings 0 = Pos.x, 1 = Seen.after; resource bindings 0 = Wind.x, 1 = Clock.ticks
DRIFT_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) { e.f32(0) = e.f32(0) + e.res_f32(0) * f.dt; e.u32(1) = e.res_u32(1); }"
# the comparison world's drift: constants where the clock world reads resources
DRIFT_PLAIN_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) { e.f32(0) = e.f32(0) + f.fparam[0] * f.dt; e.u32(1) = (ggrs_u32)f.iparam[0]; }"
BEFORE_PLAIN_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) { e.u32(0) = (ggrs_u32)f.iparam[0]; }"


def f32_bits(x):
    return int(np.array([x], dtype=F32).view(U32)[0])


def bits_f32(b):
    return np.array([b & M32], dtype=U32).view(F32)[0]


class ClockModel:
    """Clock{ticks, seed}, Wind{x (f32 bits)}, Big{acc} beside the oracle: state = [ticks, seed, wind_bits, acc]."""

    def __init__(self):
        self.cur = [CLOCK_INIT[0], CLOCK_INIT[1], f32_bits(F32(WIND_INIT)), BIG_INIT]
        self.pre = list(self.cur)
        self.snaps = {}

    def step(self, inp0, dt=DT):
        self.pre = list(self.cur)
        ticks, seed, _, acc = self.cur
        ticks = (ticks + 1) & M32
        seed = ((seed * 1664525 + 1013904223) & M32) ^ (inp0 & 0xFF)
        wind = F32(F32(seed >> 8) * WIND_SCALE) + F32(F32(dt) * WIND_BIAS)              # two products and one sum, each rounded to f32 (no contraction on the device)
        acc = (acc + 0x100000001 * seed) & M64
        self.cur = [ticks, seed, f32_bits(F32(wind)), acc]

    def save(self, frame): self.snaps[frame] = list(self.cur)

    def load(self, frame): self.cur = list(self.snaps[frame]); self.pre = list(self.cur)

    def part(self, state=None):
        """The XOR of the three ChecksumParts (resource_checksum.rs:63-83): checksum_hasher() fed each resource's chosen words in order, each with its own width."""
        s = self.cur if state is None else state
        h1 = SeaHasher(); h1.write(int(s[0]).to_bytes(4, "little")); h1.write(int(s[1]).to_bytes(4, "little"))
        h2 = SeaHasher(); h2.write(int(s[2]).to_bytes(4, "little"))
        h3 = SeaHasher(); h3.write(int(s[3]).to_bytes(8, "little"))
        return h1.finish() ^ h2.finish() ^ h3.finish()

    def words(self, state=None):
        s = self.cur if state is None else state
        return [s[0], s[1]], [s[2]], [s[3]]


def register_clock_resources(w):
    C = w.register_resource("Clock", 4, 2, CLOCK_INIT); Wn = w.register_resource("Wind", 4, 1, [f32_bits(F32(WIND_INIT))]); B = w.register_resource("Big", 8, 1, [BIG_INIT])
    w.checksum_resource(C, [0, 1]); w.checksum_resource(Wn, [0]); w.checksum_resource(B, [0])
    return C, Wn, B


def add_tick(w, res):
    C, Wn, B = res
    w.add_resource_system(TICK_SRC, [(C, 0), (C, 1), (Wn, 0), (B, 0)], fparam=(float(WIND_SCALE), float(WIND_BIAS)), name="tick")


def build_clock(w, *, model=None, plain=False, fuse_step=1):
    """Registers the clock world on `w` (a library world, or the oracle with its ClockModel); returns (Pos, Seen, Fuse).  plain: the comparison world -- no resources,
    no `tick`, `before` and `drift` reading constants (a library world only)."""
    P = w.register_component("Pos", 4, 1); S = w.register_component("Seen", 4, 2); Fz = w.register_component("Fuse", 4, 1)
    for c, words in ((P, [0]), (S, [0, 1]), (Fz, [0])): w.checksum_component(c, words)
    if isinstance(w, OracleWorld):
        def before(words, slot, f): return [model.pre[0]], 0

        def drift(words, slot, f):
            x = F32(bits_f32(words[0]) + F32(bits_f32(model.cur[2]) * F32(f.dt)))
            return [f32_bits(x), model.cur[0]], 0
        w.add_custom_system(before, [(S, 0)]); w.add_custom_system(drift, [(P, 0), (S, 1)])
    elif plain:
        w.add_custom_system(BEFORE_PLAIN_SRC, [(S, 0)], iparam=(7, 0), name="before")
        w.add_custom_system(DRIFT_PLAIN_SRC, [(P, 0), (S, 1)], iparam=(7, 0), fparam=(2.5,), name="drift")
    else:
        res = register_clock_resources(w)
        w.add_custom_system(BEFORE_SRC, [(S, 0)], name="before", resources=[(res[0], 0)])
        add_tick(w, res)
        w.add_custom_system(DRIFT_SRC, [(P, 0), (S, 1)], name="drift", resources=[(res[1], 0), (res[0], 0)])
    w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(Fz,), word=(0,), iparam=(fuse_step, bg.DESPAWN_IMMEDIATE))
    return P, S, Fz


def spawn_clock(w, ids, n, *, fuse_base=5, fuse_mod=60):
    P, S, Fz = ids
    i = np.arange(n)
    w.spawn(n, {P: [((i % 17) * 0.25 - 1.0).astype(F32).view(U32)], S: [np.zeros(n, dtype=U32), np.zeros(n, dtype=U32)], Fz: [(fuse_base + (i * 7) % fuse_mod).astype(U32)]})


def build_big(w, *, with_resources=True):
    """The in-place world: one 4-byte component under GGRS_SYS_ADD_U32 (built-in systems only on the oracle side), the clock resources and `tick`."""
    A = w.register_component("Acc", 4, 1); w.checksum_component(A, [0])
    w.add_system(bg.SYS_ADD_U32, comp=(A,), word=(0,), iparam=(3,))
    if not isinstance(w, OracleWorld) and with_resources: add_tick(w, register_clock_resources(w))
    return (A,)


def stamp(lists):
    """Every AdvanceFrame of the lists carries Time::delta_secs explicitly: the model uses the same f32."""
    for reqs in lists:
        for r in reqs:
            if isinstance(r, bg.AdvanceFrame): r.dt_bits = DT_BITS
    return lists


def synctest_lists(cd, ticks, depth=8):
    from peer_effects_common import synctest_lists as sl
    return stamp(sl(cd, ticks, depth=depth, inputs=lambda t: ((t * 5 + 3) & 15,)))


class _Recorder:
    """A world stand-in that records what a list driver (cm.P2PShapeDriver) sends: [(confirmed, requests)]."""

    def __init__(self): self.frame, self.lists, self.confirmed = 0, [], None

    def set_depth(self, d): pass

    def set_confirmed(self, c): self.confirmed = c

    def handle_requests(self, reqs):
        self.lists.append((self.confirmed, list(reqs)))
        return [0] * sum(isinstance(r, bg.SaveGameState) for r in reqs)


def p2p_lists(ticks, max_rollback=8, seed=4):
    """P2P-shaped rollbacks of 0 .. max_rollback - 1 frames (cm.P2PShapeDriver) whose inputs CHANGE between prediction and confirmation: a frame's input depends on
    the tick that simulates it, so a re-simulated frame sees another input than its first simulation -- where a wrong restore shows.  [(confirmed, requests)]."""
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
        else: model.step(int(r.inputs[0]) if len(r.inputs) else 0)
        cs = o.handle_requests([r])
        if isinstance(r, bg.SaveGameState): got.append((r.frame, cs[0] ^ model.part()))
    return got


def read_resources(w, res=(0, 1, 2)):
    return tuple(w.resource_read(r) for r in res)
