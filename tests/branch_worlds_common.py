"""Shared by the branch-step tests over wide inputs, InputStatus, Strategy, narrow-word schemas, user-written hashers and box_game (tests/test_gpu_branch_worlds.py,
tests/test_gpu_zfuzz_branch_worlds.py, tests/test_branch_worlds.py): every world on both backends, the oracle's list walk of a branch step, the one library call that
must equal it, adoption, and the fuzz tier's generator -- which the CPU tier runs with the oracle alone.

A branch step hands the library inputs[B][T][n_inputs x input_bytes] and status[B][T][n_inputs]; the library packs them into one member record per branch
(kernel_gen.hpp JitLayout::m: the n_inputs bytes, then T rows of max_players x (input_bytes + 1) bytes, unaligned).  The inputs world folds EVERY byte of a player's
input, its InputStatus and n_inputs into a checksummed word, so that one wrong byte of a row changes the branch's table."""
import ctypes as C
import multiprocessing as mp
import queue

import numpy as np

import bevy_ggrs_amd as bg
import common as cm
import test_box_game as box
import test_gpu_round5 as r5
import test_gpu_schema as sch
from oracle.binding import FLAT, OracleWorld

SAVE_LAST, RETAIN_NEWEST, RETAIN_ALL = 1, 2, 4                       # GGRS_BRANCH_* (include/ggrs_hip.h)
LAYOUTS = [(1, 2), (2, 5), (4, 3), (8, 1), (16, 3)]                  # (input_bytes, players): rows of 4, 15, 15, 9 and 51 bytes in the member record
P32 = 0x01000193                                                     # the fold's odd multiplier: s -> (s ^ v) * P32 is a bijection of s, and injective in v
M32 = 0xFFFFFFFF

# ---------------------------------------------------------------------------------------------------------------- the inputs world
_FOLD = {
    1: "    s = (s ^ (ggrs_u32)f.input[h]) * P; s = (s ^ ((ggrs_u32)f.input_u8(h) << 8)) * P;\n",
    2: "    s = (s ^ (ggrs_u32)f.input_u16(h)) * P; s = (s ^ ((ggrs_u32)f.input[h] << 16)) * P;\n",
    4: "    s = (s ^ f.input_u32(h)) * P; s = (s ^ ((ggrs_u32)f.input[h] << 8)) * P;\n",
    8: "    { const ggrs_u64 v = f.input_u64(h); s = (s ^ (ggrs_u32)v) * P; s = (s ^ (ggrs_u32)(v >> 32)) * P; }\n",
    16: "    { const unsigned char* q = f.input_ptr(h); for (int k = 0; k < 16; ++k) s = (s ^ (ggrs_u32)q[k]) * P; }\n    s = (s ^ ((ggrs_u32)f.input[h] << 8)) * P;\n",
}


def input_src(ib, const):
    """Query<(&mut Score, &Player)>: PlayerInputs<T>[player.handle] folded byte for byte (const: only player 0's first byte and status, whoever the entity is)."""
    head = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {\n    const ggrs_u32 P = 0x01000193u;\n    ggrs_u32 s = e.u32(0);\n"
    if const:
        return head + ("    if (!f.n_inputs) return;\n    s = (s ^ (ggrs_u32)f.input[0]) * P;\n    s = (s ^ (ggrs_u32)(f.input_status(0) + 1)) * P;\n"
                       "    e.u32(0) = s + f.n_inputs;\n}\n")
    return head + ("    const int h = (int)e.u64(1);\n    if (h >= (int)f.n_inputs) return;\n" + _FOLD[ib] +
                   "    s = (s ^ (ggrs_u32)(f.input_status(h) + 1)) * P;\n    e.u32(0) = s + f.n_inputs;\n}\n")


def input_twin(ib, const, stats):
    """The same system for the oracle.  stats["status"][k]: how often an entity saw InputStatus k (every entity of this world lives)."""
    def fold(s, v): return ((s ^ v) * P32) & M32

    def fn(words, slot, f):
        s, h, ni = words[0] & M32, words[1], f.n_inputs
        if const:
            if not ni: return words, 0
            st = f.status[0]
            s = fold(fold(s, f.input(0)[0]), st + 1)
        else:
            if h >= ni: return words, 0
            b = f.input(h); st = f.status[h]
            if ib == 1: s = fold(fold(s, b[0]), b[0] << 8)
            elif ib == 2: s = fold(fold(s, int.from_bytes(b, "little")), b[0] << 16)
            elif ib == 4: s = fold(fold(s, int.from_bytes(b, "little")), b[0] << 8)
            elif ib == 8: s = fold(fold(s, int.from_bytes(b[:4], "little")), int.from_bytes(b[4:], "little"))
            else:
                for k in range(16): s = fold(s, b[k])
                s = fold(s, b[0] << 8)
            s = fold(s, st + 1)
        stats["status"][st] += 1
        return [(s + ni) & M32, h], 0
    return fn


def build_inputs(w, n, ib, players, const, stats):
    w.set_input_layout(ib, players)
    S = w.register_component("Score", 4, 1)
    H = w.register_component("Player", 8, 1)
    w.checksum_component(S, [0])
    w.add_custom_system(input_twin(ib, const, stats) if isinstance(w, OracleWorld) else input_src(ib, const), [(S, 0), (H, 0)], name="score")
    w.spawn(n, {S: [np.arange(n, dtype=np.uint32) * 2654435761 & M32], H: [(np.arange(n) % (players + 1)).astype(np.uint64)]})      # handle == players: never an input
    return S, H


# ---------------------------------------------------------------------------------------------------------------- the other worlds
ADD_INPUT_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) { e.u32(0) += f.n_inputs ? (ggrs_u32)f.input[0] : 0u; }"


def add_input_twin(words, slot, f):
    return [(words[0] + (f.input(0)[0] if f.n_inputs else 0)) & M32], 0


def _add_input(w, comp, word):
    """One small input-dependent system, so that branches diverge: word += PlayerInputs[0]."""
    w.add_custom_system(add_input_twin if isinstance(w, OracleWorld) else ADD_INPUT_SRC, [(comp, word)], name="add_input")


def build_strategy(w, n):
    """test_gpu_round5._f16_world (Accel.x exact in f16, Accel.y lossy, Accel.z never written) + Count += input."""
    A, C_ = r5._f16_world(w, True)
    _add_input(w, C_, 0)
    rng = np.random.default_rng(5)
    x = (rng.integers(-40, 40, n) * 0.5).astype(np.float32); y = rng.uniform(1, 2, n).astype(np.float32); z = rng.uniform(-1000, 1000, n).astype(np.float32)
    w.spawn(n, {A: [cm.f32bits(x), cm.f32bits(y), cm.f32bits(z)], C_: [np.zeros(n, dtype=np.uint32)]})
    return A, C_


BOX_CHECKSUMS = ((0, [0, 1, 2]), (1, [0, 1, 2]))                     # translation and velocity: what move_cube_system writes

KINDS = [("inputs", l) for l in LAYOUTS] + [("const", (1, 2)), ("const", (16, 3)), ("strategy", (1, 16)), ("narrow", (1, 16)), ("hasher", (1, 16)), ("box", (1, 2)), ("box", (1, 4))]
PY_KINDS = ("inputs", "const", "strategy", "narrow", "hasher")      # the oracle side runs Python callbacks per entity


def players_of(kind, layout):
    """How many players a step of this world may carry (box_game: the cubes' handles; the worlds that read player 0 alone: 2)."""
    return layout[1] if kind in ("inputs", "const", "box") else 2


def new_stats():
    return {"status": [0, 0, 0]}


def build_world(w, kind, layout, n, stats):
    """-> the component ids whose columns make up the observable state"""
    ib, players = layout
    if kind in ("inputs", "const"): return build_inputs(w, n, ib, players, kind == "const", stats)
    if kind == "strategy": return build_strategy(w, n)
    if kind == "narrow": return sch.build_narrow(w, n, extra=lambda w_, ids: _add_input(w_, ids[2], 0))
    if kind == "hasher": return sch.build_odd_hasher(w, n, extra=lambda w_, ids: _add_input(w_, ids[0], 0))
    if kind == "box": return box.build_box(w, n, players, spread=True, checksums=BOX_CHECKSUMS)[0]
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------- requests
def advance(inp, st, n_inputs, ib):
    """AdvanceFrame of one frame's PlayerInputs: inp[P][ib] bytes, st[P] InputStatus bytes or None."""
    ins = tuple(int(inp[p, 0]) if ib == 1 else bytes(inp[p].tobytes()) for p in range(n_inputs))
    return bg.AdvanceFrame(ins, status=None if st is None or not n_inputs else tuple(int(x) for x in st[:n_inputs]))


def branch_requests(F, inp, st, n_inputs, ib, k, save_last, saves=True):
    """[Load(F), (Advance, Save) ..] of one branch, its first k frames of T; saves=False: the Advances only."""
    T = inp.shape[0]
    reqs = [bg.LoadGameState(F)]
    for i in range(k):
        reqs.append(advance(inp[i], None if st is None else st[i], n_inputs, ib))
        if saves and (i < T - 1 or save_last): reqs.append(bg.SaveGameState(F + 1 + i))
    return reqs


def adoption_requests(F, inp, st, n_inputs, ib, k):
    """What include/ggrs_hip.h documents ggrs_hip_fanout_adopt(branch, F + k) to equal: "that branch's retained state of `frame` becomes the world -- ... a snapshot
    of `frame` in the ring, the live world loaded from it (what LoadGameState leaves behind)": the branch's replay, then SaveGameState(F + k), LoadGameState(F + k)."""
    return branch_requests(F, inp, st, n_inputs, ib, k, False, saves=False) + [bg.SaveGameState(F + k), bg.LoadGameState(F + k)]


def oracle_walk(ow, prefix, inputs, status, n_inputs, save_last):
    """The list form: the prefix, every branch as its own request list, and the LoadGameState(F) that leaves the world where the branches started.
    -> (F, the prefix's checksums, one list of checksums per branch)"""
    B = inputs.shape[0]
    pre = list(ow.handle_requests(prefix))
    F = ow.frame
    per = [list(ow.handle_requests(branch_requests(F, inputs[b], None if status is None else status[b], n_inputs, ow.input_bytes, inputs.shape[1], save_last))) for b in range(B)]
    ow.handle_requests([bg.LoadGameState(F)])
    return F, pre, per


def library_step(native, gw, prefix, inputs, status, n_inputs, flags):
    """ggrs_hip_fanout_step_branches + collect: (rc, this step's Checksum(u128)s) or (rc, the error text).  inputs[B][T][P][ib] u8 (P >= n_inputs: the first
    n_inputs players travel), status[B][T][P] u8 or None; n_inputs = 0 passes inputs = NULL."""
    from bevy_ggrs_amd import _ffi
    B, T = inputs.shape[:2]
    pre, keep, _ = gw.build_requests(prefix)
    bs = _ffi.BranchStep()
    bs.prefix, bs.n_prefix, bs.n_branches, bs.n_frames, bs.n_inputs, bs.flags = pre, len(prefix), B, T, n_inputs, flags
    inp = np.ascontiguousarray(inputs[:, :, :n_inputs], dtype=np.uint8)
    st = None if status is None else np.ascontiguousarray(status[:, :, :n_inputs], dtype=np.uint8)
    if n_inputs: bs.inputs = inp.ctypes.data
    if st is not None and n_inputs: bs.status = st.ctypes.data
    ns = C.c_uint32(0)
    rc = _ffi.lib.ggrs_hip_fanout_step_branches(native._p, C.byref(bs), C.byref(ns))
    if rc != 0:
        return rc, (_ffi.lib.ggrs_hip_fanout_last_error(native._p) or b"").decode()
    got = [int(p[0]) | (int(p[1]) << 64) for p in native.collect().reshape(-1, 2)]
    assert ns.value == len(got), (ns.value, len(got))
    return 0, got


def run_in_process(target, *args, timeout=900):
    """target(q, *args) in a spawned process (its own HIP context and RCCL communicators); -> what it put on q.  A process that ends without a report is an error at
    once, not after the timeout."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=target, args=(q,) + args); p.start()
    r, waited = None, 0
    try:
        while r is None:
            try: r = q.get(timeout=2)
            except queue.Empty:
                waited += 2
                if not p.is_alive():
                    try: r = q.get(timeout=2)
                    except queue.Empty: r = ("error", f"the process ended with exit code {p.exitcode} and left no report")
                elif waited >= timeout: r = ("error", f"no report after {timeout} s")
    finally:
        p.join(timeout=30)
        if p.is_alive(): p.kill()
    return r


# ---------------------------------------------------------------------------------------------------------------- one world on the oracle and, if asked, the library
class Session:
    def __init__(self, kind, layout, n, depth, with_lib, vtags=0, lazy=0):
        self.kind, self.layout, self.n, self.depth, self.stats = kind, layout, n, depth, new_stats()
        self.ib, self.players = layout[0], players_of(kind, layout)
        self.what = dict(kind=kind, layout=layout, n=n, depth=depth, vtags=vtags, lazy=lazy)
        self.ow = OracleWorld(n + 8, depth + 2, FLAT)
        self.gw = self.native = None
        if with_lib:
            from bevy_ggrs_amd import _ffi
            from bevy_ggrs_amd.fanout import RcclFanout
            self.gw = bg.World(n + 8, max_depth=depth + 2)
            if vtags: assert _ffi.lib.ggrs_dbg_set_value_tags(self.gw._p, 1) == 0
            if lazy: assert _ffi.lib.ggrs_dbg_set_lazy_live(self.gw._p, lazy) == 0
        for w in self.worlds():
            self.ids = build_world(w, kind, layout, n, self.stats)
            w.set_depth(depth + 1)
        if with_lib: self.native = RcclFanout(self.gw, 0, 1, RcclFanout.unique_id())
        self.last = self.saves = None

    def worlds(self):
        return [w for w in (self.gw, self.ow) if w is not None]

    def rand_inputs(self, rng, B, T):
        """inputs[B][T][players][ib]: box_game reads four bits per player, everybody else every bit"""
        return rng.integers(0, 16 if self.kind == "box" else 256, size=(B, T, self.players, self.ib)).astype(np.uint8)

    def rand_advance(self, rng, n_inputs, with_status=True):
        inp = self.rand_inputs(rng, 1, 1)[0, 0]
        return advance(inp, rng.integers(0, 3, self.players) if with_status else None, n_inputs, self.ib)

    def agree(self, prefix, B, T, flags):
        """Every step of one fan-out holds the same number of SaveGameStates; a step of another shape starts a new agreement (ggrs_hip_fanout_set_interval)."""
        saves = sum(isinstance(r, bg.SaveGameState) for r in prefix) + B * (T if flags & SAVE_LAST else T - 1)
        if self.native is not None and self.saves not in (None, saves): self.native.set_interval(1)
        self.saves = saves

    def same_state(self, ctx):
        if self.gw is None: return
        assert self.gw.frame == self.ow.frame and self.gw.len == self.ow.len, (self.what, ctx, self.gw.frame, self.ow.frame, self.gw.len, self.ow.len)
        cm.assert_states_equal(cm.snapshot_state(self.gw, self.ids), cm.snapshot_state(self.ow, self.ids), f"{self.what} {ctx}")

    def step(self, prefix, inputs, status, n_inputs, flags, ctx=""):
        """One branch step on both: the table, the live state, the frame and len are the oracle's.  -> the oracle's checksums per branch"""
        for w in self.worlds(): w.set_confirmed(w.frame)
        F, pre, per = oracle_walk(self.ow, prefix, inputs, status, n_inputs, bool(flags & SAVE_LAST))
        if self.gw is not None:
            want = pre + [c for b in per for c in b]
            self.agree(prefix, inputs.shape[0], inputs.shape[1], flags)
            rc, got = library_step(self.native, self.gw, prefix, inputs, status, n_inputs, flags)
            assert rc == 0, (self.what, ctx, rc, got)
            assert len(got) == len(want), (self.what, ctx, len(got), len(want))
            bad = [k for k in range(len(want)) if want[k] != got[k]]
            assert not bad, (self.what, ctx, "first differing Checksum(u128) at", bad[0], "of", len(want), "prefix", len(pre), "per branch", len(per[0]))
            assert self.gw.frame == F, (self.what, ctx, self.gw.frame, F)
            self.same_state(f"{ctx}: after the step")
        self.last = (F, inputs, status, n_inputs, flags)
        return per

    def refused(self, prefix, inputs, status, n_inputs, flags):
        """A step that validate_branch_step refuses: -> (rc, message); the world has not moved."""
        frame, ln = self.gw.frame, self.gw.len
        self.agree(prefix, inputs.shape[0], inputs.shape[1], flags)
        rc, msg = library_step(self.native, self.gw, prefix, inputs, status, n_inputs, flags)
        assert rc != 0, (self.what, "accepted", flags)
        assert self.gw.frame == frame and self.gw.len == ln, (self.what, "a refused step moved the world", self.gw.frame, frame, self.gw.len, ln)
        return rc, msg

    def adopt(self, b, k, tick_inputs=None):
        """Branch b of the last step at its k-th frame becomes the world; then one ordinary tick.  -> the state fields in which the documented list differs from the
        plain replay (a lossy Strategy's words: decided on the oracle alone)."""
        F, inputs, status, n_inputs, flags = self.last
        st = None if status is None else status[b]
        if self.native is not None: self.native.adopt(b, F + k)
        self.ow.handle_requests(branch_requests(F, inputs[b], st, n_inputs, self.ib, k, False, saves=False))
        plain = cm.snapshot_state(self.ow, self.ids)
        self.ow.handle_requests(adoption_requests(F, inputs[b], st, n_inputs, self.ib, k))
        doc = cm.snapshot_state(self.ow, self.ids)
        lossy = sorted(key for key, v in doc.items() if isinstance(v, np.ndarray) and not np.array_equal(v, plain[key]))
        self.same_state(f"adopted branch {b} at +{k}")
        if self.gw is not None: assert self.gw.save() == self.ow.save(), (self.what, "SaveGameState after adoption", b, k)
        for w in self.worlds(): w.set_confirmed(w.frame)
        a = tick_inputs if tick_inputs is not None else bg.AdvanceFrame(())
        t1 = [bg.SaveGameState(F + k), a, bg.SaveGameState(F + k + 1)]
        cs = [list(w.handle_requests(t1)) for w in self.worlds()]
        assert all(c == cs[-1] for c in cs), (self.what, "the tick after adoption", b, k)
        self.same_state(f"the tick after adopting branch {b} at +{k}")
        return lossy

    def close(self):
        if self.native is not None: self.native.close()
        for w in self.worlds():
            if hasattr(w, "close"): w.close()


# ---------------------------------------------------------------------------------------------------------------- the fuzz tier's generator
FUZZ_SEEDS = list(range(7300, 7336))                                 # seed i runs KINDS[i % 12]: a chunk (seeds[c::3]) meets four kinds, each in that chunk alone


def fuzz_seed(seed, with_lib):
    """One seed of tests/test_gpu_zfuzz_branch_worlds.py: three consecutive branch steps behind a prefix, then -- where the step retained -- adoption of a random
    retained frame and the tick after.  with_lib=False: the oracle alone (tests/test_branch_worlds.py counts the floors from what this returns)."""
    rng = np.random.default_rng(seed)
    i = seed - FUZZ_SEEDS[0]
    kind, layout = KINDS[i % len(KINDS)]
    py = kind in PY_KINDS
    n = int(rng.choice([40, 300, 1500] if py else [40, 300, 1500, 6000]))
    depth = int(rng.integers(3, 9))
    T = int(rng.integers(1, depth + 1))
    B = int(rng.choice([1, 2, 5] if py and n == 1500 else [1, 2, 5, 17]))      # (the callbacks of 17 branches x 1500 entities would take the CPU tier a minute)
    save_last = bool(rng.integers(0, 2)) or T == 1
    retain = int(rng.choice([0, RETAIN_NEWEST, RETAIN_ALL]))
    if kind == "strategy" and retain: save_last = True                           # a Strategy world keeps branch states only as snapshots
    flags = (SAVE_LAST if save_last else 0) | retain
    with_status = bool(seed % 3)                                                 # NULL for a third of the seeds
    odd = bool(seed % 2)
    s = Session(kind, layout, n, depth, with_lib, vtags=int(odd), lazy=(2 if seed % 4 == 1 else 1) if odd else 0)
    rec = dict(seed=seed, kind=kind, layout=layout, n=n, depth=depth, T=T, B=B, flags=flags, with_status=with_status, steps=[], adopted=None, lossy=False, stats=s.stats)
    s.what.update(seed=seed, T=T, B=B, flags=flags)
    warm = advance(np.zeros((s.players, s.ib), dtype=np.uint8), None, 1, s.ib)
    for w in s.worlds(): w.handle_requests([warm, warm])
    for step in range(3):
        Cf = s.ow.frame
        n_inputs = 0 if rng.integers(0, 16) == 0 else int(rng.integers(1, s.players + 1))
        prefix = [bg.SaveGameState(Cf)] if step == 0 else [bg.LoadGameState(Cf), s.rand_advance(rng, int(rng.integers(1, s.players + 1)), with_status), bg.SaveGameState(Cf + 1)]
        inputs = s.rand_inputs(rng, B, T)
        status = rng.integers(0, 3, size=(B, T, s.players)).astype(np.uint8) if with_status else None
        per = s.step(prefix, inputs, status, n_inputs, flags, ctx=f"step {step}")
        rec["steps"].append(dict(n_inputs=n_inputs, distinct=len({tuple(p) for p in per}), saves=len(per[0])))
    if retain:
        b = int(rng.integers(0, B))
        k = int(rng.integers(1, T + 1)) if retain == RETAIN_ALL else T
        rec["lossy"] = bool(s.adopt(b, k, s.rand_advance(rng, 1, with_status)))
        rec["adopted"] = (b, k)
    s.close()
    return rec
