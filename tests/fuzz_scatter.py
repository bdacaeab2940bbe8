"""Bulk host edits under the request fuzzer (fuzz_util.run(scenario=..., ring_sweep=True)): scenario subclasses of the particles and generic families and of the
skirmish world whose extra_edit(x, A, B, ids) draws a scatter -- an op and a row set -- and applies it to the oracle A one slot at a time
(scatter_common.apply_per_slot) and to B through ONE scatter call.  Existing scenarios are left alone: their seeds' streams do not move.

A row set is a random ascending subset of up to 256 slots of [0, len), dead slots and slots without the named component left in: either spread over the whole
world or dense inside a window (so that rows of one 64-slot unit land in two waves).  One draw in twelve plants a bad row -- a duplicate, a descending pair or a
slot at or beyond len -- which both sides must refuse without changing anything.

Beside the fuzzer's own comparisons (checksums, the state, the ring sweep) every edit compares the two reports and holds B to what the state comparison cannot
see: the words, presence bits and alive bits of the rows that were NOT applied -- dead slots, slots without the component, every row of a refused call -- are read
back raw from B before and after the call and must not have moved.

What a session covered is counted from the oracle's side alone (Coverage): test_fuzz_scatter.py holds the committed seeds to floors with it.
(A helper module, no tests of its own.)"""
from collections import Counter

import numpy as np

import bevy_ggrs_amd as bg
import common as cm
import fuzz_user_worlds as fu
import fuzz_util
import query_common as qc
import scatter_common as sc
from oracle.binding import FLAT, OracleWorld

U8, U16, U32, U64, F32 = np.uint8, np.uint16, np.uint32, np.uint64, np.float32
MAX_ROWS = 256
P_OP = (("write", 0.40), ("insert", 0.25), ("remove", 0.20), ("despawn", 0.15))
P_BAD = 1 / 12


class BulkEdits:
    """What the three scenarios share: the draw, the two applications, the raw check and the count of what was covered.  A scenario says which components take
    part (bulk_comps) and what their words may hold (bulk_col)."""

    def _bulk_init(self): self.cov, self.n_bulk = Counter(), 0

    def bulk_comps(self, ids): return list(ids)

    def bulk_col(self, A, comp, k, m):
        wb = A._comps[comp][1]
        return self.rng.integers(0, 2 ** (8 * wb), m, dtype=U64).astype(qc.UINT[wb])

    def draw_rows(self, n, op):
        r = self.rng
        cap = min(n, MAX_ROWS if op != "despawn" else 24)                        # (despawns thin the world: a few at a time)
        if r.random() < 0.5:
            k = int(r.integers(0, cap + 1))
            slots = np.sort(r.choice(n, k, replace=False)) if k else np.zeros(0, dtype=np.int64)
        else:
            start = int(r.integers(0, n)); span = int(r.integers(1, 2 * cap + 2))
            win = np.arange(start, min(n, start + span))
            slots = win[r.random(win.size) < 0.85][:cap]
        slots = slots.astype(np.int64)
        bad = None
        if r.random() < P_BAD and slots.size >= 2:
            i = int(r.integers(1, slots.size)); bad = ("duplicate", "descending", "beyond len")[int(r.integers(0, 3))]
            if bad == "duplicate": slots[i] = slots[i - 1]
            elif bad == "descending": slots[i - 1], slots[i] = slots[i], slots[i - 1]
            else: slots[i] = n + int(r.integers(0, 3))
        return slots, bad

    def draw_bulk(self, A, ids):
        r, n = self.rng, A.len
        x, op = r.random(), None
        for name, p in P_OP:
            if x < p: op = name; break
            x -= p
        op = op or "despawn"
        comps = self.bulk_comps(ids)
        words, named = [], []
        if op == "write":
            for c in [comps[int(i)] for i in r.choice(len(comps), min(len(comps), int(r.integers(1, 3))), replace=False)]:
                nw = A._comps[c][2]
                words += [(c, int(k)) for k in r.choice(nw, int(r.integers(1, nw + 1)), replace=False)]
            words = words[:qc_max()]
        elif op == "insert":
            c = comps[int(r.integers(len(comps)))]
            words = [(c, k) for k in range(A._comps[c][2])]
            if r.random() < 0.5: words.reverse()
        elif op == "remove":
            named = [comps[int(i)] for i in r.choice(len(comps), min(len(comps), int(r.integers(1, 3))), replace=False)]
        slots, bad = self.draw_rows(n, op)
        cols = [self.bulk_col(A, c, k, slots.size) for c, k in words]
        return sc.make_sdesc(op, words, named), slots, cols, bad

    def extra_edit(self, x, A, B, ids):
        n = A.len
        if not n: return None
        desc, slots, cols, bad = self.draw_bulk(A, ids)
        op = desc["op"]
        named = sorted({c for c, _ in desc["words"]} | desc["comps"])
        in_flight = bool(B.pending_batches()) if hasattr(B, "pending_batches") else False
        # what the state comparison cannot see: B's raw words and bits at the rows, before the call
        raw = lambda: ({key: B.download_word(key[0], key[1], 0, n) for key in desc["words"]}, {c: B.present_mask(c, n) for c in named}, B.alive_mask(n))
        w0, p0, a0 = raw()
        rec = sc.mask_record(A, named)
        valid = sc.first_bad_row(n, slots) is None
        assert valid == (bad is None)
        applied = sc.verdicts(rec, desc, slots)[0] if valid else np.zeros(slots.size, dtype=bool)
        want = sc.apply_per_slot(A, desc, slots, cols)
        got = sc.world_scatter(B, desc, slots, cols)
        ctx = f"{self.describe()}: scatter {op} of {slots.size} rows ({bad or 'valid'}), words {desc['words']}, comps {sorted(desc['comps'])}"
        assert got == want, f"{ctx}: the reports differ: {got} vs {want}"
        w1, p1, a1 = raw()
        idle = slots[~applied]
        idle = idle[idle < n]
        for key in w0: assert np.array_equal(w0[key][idle], w1[key][idle]), f"{ctx}: word {key} of a row that was not applied moved (slots {idle[w0[key][idle] != w1[key][idle]][:8]})"
        for c in p0: assert np.array_equal(p0[c][idle], p1[c][idle]), f"{ctx}: the presence bit of component {c} of a row that was not applied moved"
        assert np.array_equal(a0[idle], a1[idle]), f"{ctx}: the alive bit of a row that was not applied moved"
        on = slots[applied]                                                      # ... and the rows that were applied hold what the op says, at once
        for key, col in zip(desc["words"], cols): assert np.array_equal(w1[key][on], col[applied]), f"{ctx}: word {key} of an applied row does not hold its value"
        if op == "insert": assert all(p1[c][on].all() for c in p1), f"{ctx}: an applied row lacks the presence bit of the inserted component"
        if op == "remove": assert not any(p1[c][on].any() for c in p1), f"{ctx}: an applied row kept the presence bit of a removed component"
        if op == "despawn": assert not a1[on].any(), f"{ctx}: an applied row is still alive"
        # coverage, from the oracle's verdicts alone
        self.n_bulk += 1
        cov = self.cov
        cov[op] += 1
        if want["n_dead"]: cov["dead"] += 1
        if want["n_absent"]: cov["absent"] += 1
        if bad: cov["bad"] += 1
        if in_flight: cov["in_flight"] += 1
        if valid and slots.size > 64:
            i = np.arange(64, slots.size, 64)
            if (slots[i] // 64 == slots[i - 1] // 64).any(): cov["two_waves"] += 1
        return f"scatter {op} rows={slots.size} applied={want['n_applied']} dead={want['n_dead']} absent={want['n_absent']}" + (f" REFUSED at row {want['first_bad_row']} ({bad})" if bad else "") + (" (in flight)" if in_flight else "")


def qc_max(): return 32                                                          # GGRS_QUERY_MAX_WORDS


class ParticlesScatter(BulkEdits, fuzz_util.Scenario):
    """The particles family: Transform and Velocity take finite floats (the step integrates them), Ttl a count of frames."""

    def __init__(self, seed, *, big=False, max_n=None):
        fuzz_util.Scenario.__init__(self, seed, big=big, max_n=max_n); self._bulk_init()

    def describe(self): return "scatter " + fuzz_util.Scenario.describe(self)

    def bulk_comps(self, ids): return list(ids[:3])

    def bulk_col(self, A, comp, k, m):
        if A._comps[comp][1] == 8: return self.rng.integers(1, 300, m).astype(U64)
        return cm.f32bits(self.rng.uniform(-100, 100, m).astype(F32))


class GenericScatter(BulkEdits, fuzz_util.GenericScenario):
    """The generic family: words of every width hold random bits; a component outside rollback and Health are rows like any other."""

    def __init__(self, seed, *, big=False, max_n=None, plain=False):
        fuzz_util.GenericScenario.__init__(self, seed, big=big, max_n=max_n, plain=plain); self._bulk_init()

    def describe(self): return "scatter " + fuzz_util.GenericScenario.describe(self)


class SkirmishScatter(BulkEdits, fu.SkirmishScenario):
    """The skirmish world: words as its own host edits draw them (finite floats in Pos, links that mostly name an entity)."""

    def __init__(self, seed, n=None):
        fu.SkirmishScenario.__init__(self, seed, n=n); self._bulk_init()

    def describe(self): return "scatter " + fu.SkirmishScenario.describe(self)

    def bulk_col(self, A, comp, k, m): return self._col(self.ids.index(comp), k, m)

    def extra_edit(self, x, A, B, ids):
        if x >= 0.94: return fu.SkirmishScenario.extra_edit(self, 0.0, A, B, ids)       # (the world's own edit now and then: Energy)
        return BulkEdits.extra_edit(self, x, A, B, ids)


# ---- the committed cases: family -> (scenario, keywords of fuzz_util.run, seeds); the GPU tier and the CPU tier both read these ----------------------------------------
SMALL = 1100                                                                     # the sizes up to 1000 (the skirmish: up to 1025)
FAMILIES = {
    "particles": dict(cls=ParticlesScatter, max_n=SMALL, n_lists=30),
    "generic": dict(cls=GenericScatter, max_n=SMALL, n_lists=30),
    "generic_plain": dict(cls=GenericScatter, max_n=SMALL, n_lists=30, kw={"plain": True}),      # (stays eligible for deferred Saves for a whole session)
    "skirmish": dict(cls=SkirmishScatter, max_n=None, n_lists=20),
    "particles_tile": dict(cls=ParticlesScatter, max_n=8300, n_lists=14),
    "generic_tile": dict(cls=GenericScatter, max_n=8300, n_lists=14),
}
# mode: how the device world of the GPU tier is set up (the CPU tier runs every case the same way)
CASES = {
    "default": [("particles", s) for s in (0, 1, 2, 3, 4)] + [("generic", s) for s in (0, 1, 2, 3, 4)] + [("skirmish", s) for s in (0, 1, 2, 3, 4, 5)],
    "tags_lazy": [("particles", s) for s in (10, 11, 12, 13)] + [("generic", s) for s in (10, 11, 12, 13)],
    "deferral": [("particles", s) for s in (20, 21, 22, 23)] + [("generic_plain", s) for s in (20, 21, 22, 23)],
    "tile": [("particles_tile", s) for s in (12, 21)] + [("generic_tile", s) for s in (4, 8)],        # (the seeds that draw n = 8193)
}
ALL_CASES = [(mode, fam, seed) for mode, cases in CASES.items() for fam, seed in cases]
TILE_MIN = 8193                                                                  # a tile case's world reaches across slot 8192


def group(family): return family.replace("_tile", "").replace("_plain", "")


def run_case(family, seed, make_b, **kw):
    """fuzz_util.run of one committed case with the FLAT oracle (adapter) as backend A; returns (log, scenario)."""
    fam, seen = FAMILIES[family], {}

    def scenario(seed_, big, max_n):
        seen["sc"] = fam["cls"](seed_) if fam["cls"] is SkirmishScatter else fam["cls"](seed_, max_n=fam["max_n"], **fam.get("kw", {}))
        return seen["sc"]

    def make_a(sc_): return sc_.oracle(FLAT) if hasattr(sc_, "oracle") else OracleWorld(sc_.capacity, 8, FLAT)

    def extra(w): return seen["sc"].extra_state(w) if hasattr(seen["sc"], "extra_state") else {}
    log = fuzz_util.run(seed, make_a, make_b, scenario=scenario, ring_sweep=True, n_lists=fam["n_lists"], extra_state=extra, **kw)
    return log, seen["sc"]


def rolled_back(log):
    """How many scatter edits of a log a later Load took back: a Load of a frame whose last Save stands before the edit (the ring sweep's Loads count)."""
    saved, edits, hit, pos = {}, [], set(), 0
    for line in log[1:]:
        toks = line.replace("(enqueued)", "").replace("(sweep)", "").split()
        if line.startswith("scatter ") and "REFUSED" not in line and " applied=0 " not in line:
            edits.append(pos); pos += 1
            continue
        if not toks or not all(fuzz_util._TOK.match(t) for t in toks): continue
        for t in toks:
            pos += 1
            if t[0] == "S": saved[int(t[1:])] = pos
            elif t[0] == "L":
                at = saved.get(int(t[1:]), -1)
                hit |= {e for e in edits if e > at}
                edits = [e for e in edits if e <= at]
    return len(hit)
