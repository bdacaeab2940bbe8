"""The census world (peer_index_common.py) as a scenario of the request fuzzer (fuzz_util.run(scenario=...)), with OracleAdapter reused from fuzz_user_worlds.py.

What the scripted sessions never send and the fuzzer does: lists in any order, one frame loaded and advanced many times inside one list, Saves that evict their
own source, the depth and ConfirmedFrameCount moving, and host edits between lists and BEHIND lists in flight -- upload_word on the key (one value in four out of
range), insert / remove of the key component, despawn.  Every AdvanceWorld of this world is a launch of its own with a publish and an index build ahead of it: a
Load in the middle of a list, or an edit behind a list in flight, is where yesterday's index would show.

The adapter counts, on the oracle alone, what the coverage floors of test_fuzz_peer_index.py are held to:
    multi        AdvanceFrames whose start-of-frame index has a bucket with two members at least (a system observes it: every member runs the census)
    out_of_range AdvanceFrames at whose start a visible entity's key is >= n_buckets
    lost         host edits between lists that take a member out of the index (a despawn, a removed key component, a key uploaded out of range)
    load_differs Loads followed by an AdvanceFrame whose index (the loaded frame's) differs from the live world's just before the Load
(A helper module, no tests of its own.)"""
import hashlib

import numpy as np

import bevy_ggrs_amd as bg
import fuzz_user_worlds as fu
import fuzz_util
from oracle.binding import FLAT, REFSHAPED, OracleWorld
from peer_index_common import build_census, model_index, spawn_census

U32 = np.uint32
SIZES = fu.SIZES
RUN_KW = {"n_lists": 20, "ring_sweep": True}
SEEDS = range(24)                      # the device sessions; with TILE the 25 the GPU tier runs
TILE = (3, 8262, 5)                    # (seed, n, n_lists): one session across the 8192-slot layout tile


class Stats:
    def __init__(self): self.multi = self.out_of_range = self.lost = self.load_differs = self.advances = 0


class CensusAdapter(fu.OracleAdapter):
    """OracleAdapter (no model, no hooks) that looks at the index of the oracle's state around what it hands on."""

    def _members(self):
        o, K = self.oracle, self.ids[0]
        n = o.len
        if not n: return np.zeros(0, dtype=bool), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
        vis = o.alive_mask(n) & o.present_mask(K, n)
        key = o.download_word(K, 0, 0, n).astype(np.int64)
        return vis & (key < self.nb), key, vis

    def _sig(self):
        o, K = self.oracle, self.ids[0]
        n = o.len
        if not n: return b""
        st, sl = model_index(o.alive_mask(n), o.present_mask(K, n), o.download_word(K, 0, 0, n), n, self.nb)
        return hashlib.sha256(st.tobytes() + sl.tobytes()).digest()

    def one(self, r):
        st = self.stats
        if isinstance(r, bg.AdvanceFrame):
            mem, key, vis = self._members()
            st.advances += 1
            st.multi += bool(mem.any() and np.bincount(key[mem], minlength=1).max() >= 2)
            st.out_of_range += bool((vis & (key >= self.nb)).any())
            if self.__dict__.get("after_load") is not None:
                st.load_differs += self.after_load[0] != self.after_load[1]
        self.__dict__["after_load"] = None
        if isinstance(r, bg.LoadGameState):
            before = self._sig()
            out = self.oracle.handle_requests([r])
            self.__dict__["after_load"] = (before, self._sig())
            return out
        return self.oracle.handle_requests([r])

    def _edit(self, name, *a):
        before = self._members()[0]
        getattr(self.oracle, name)(*a)
        after = self._members()[0]
        m = min(before.size, after.size)
        self.stats.lost += bool((before[:m] & ~after[:m]).any())

    def despawn(self, s): self._edit("despawn", s)
    def remove_component(self, c, s): self._edit("remove_component", c, s)
    def upload_word(self, c, k, first, data): self._edit("upload_word", c, k, first, data)
    def insert_component(self, c, s, w): self._edit("insert_component", c, s, w)


class CensusScenario(fu._UserScenario):
    """peer_index_common.build_census under random request lists: n from SIZES (or pinned), n_buckets drawn from 3 / 40 / 300 (one radix pass or two; crowded or
    sparse buckets), depth 1..8.  Keys written by the host are in range three times out of four."""
    with_spawn, spawn_budget = False, 0
    #        Key       Out             Hp
    cols = (("key",), ("u32",) * 8, ((1, 200),))

    def __init__(self, seed, n=None):
        self._common(0x1DE8, seed, n)
        self.nb = int(self.rng.choice((3, 40, 300)))

    def describe(self): return f"census seed {self.seed}: n={self.n} n_buckets={self.nb} depth={self.depth}"

    def _col(self, comp, k, m):
        if self.cols[comp][k] != "key": return super()._col(comp, k, m)
        r = self.rng
        inside = r.integers(0, self.nb, m); outside = self.nb + r.integers(0, 1 << 20, m)
        return np.where(r.random(m) < 0.25, outside, inside).astype(U32)

    def oracle(self, mode):
        return CensusAdapter(OracleWorld(self.capacity, 8, mode), None, Stats(), False, False, nb=self.nb, ids=None, after_load=None)

    def build(self, world):
        target = world.oracle if hasattr(world, "oracle") else world
        ids = build_census(target, self.nb)
        adapter = world._w if isinstance(world, fu.InFlight) else world
        if hasattr(world, "oracle"): adapter.__dict__["ids"] = tuple(ids)
        spawn_census(target, ids, self.n, self.nb, n_bare=self.n // 8)
        return self._finish(world, ids)

    def advance(self, frame, spawn): return bg.AdvanceFrame((int(self.rng.integers(0, 4)),))


def factory(n=None):
    return lambda seed, big, max_n: CensusScenario(seed, n=n)


def run(seed, make_b, *, n=None, on_end=None, after_list=None, **kw):
    """fuzz_util.run of one committed case with the FLAT adapter as backend A; returns (log, scenario, A's Stats)."""
    seen = {}

    def make_a(sc): seen["sc"] = sc; seen["A"] = sc.oracle(FLAT); return seen["A"]
    log = fuzz_util.run(seed, make_a, make_b, scenario=factory(n), on_end=on_end, after_list=after_list, **{**RUN_KW, **kw})
    return log, seen["sc"], seen["A"].stats


def cpu_pair(seed, **kw):
    """The generator guard: the FLAT adapter against the REFSHAPED one behind InFlight -- the stream the HIP backend gets."""
    return run(seed, lambda sc: fu.InFlight(sc.oracle(REFSHAPED)), **kw)
