"""A witness for the request fuzzers (fuzz_util.run(witness=...)): the inspection calls -- World.checksum_parts, World.diff, World.query, World.snapshot_copy -- asked
about the live world and about every ring frame of random sessions, and held to the three numpy models (checksum_parts_common.model_parts, state_diff_common.model_diff,
query_common.model_of / expected_buffer) over what the ORACLE says those states are.

The model inputs come from backend A alone: its live world where A and B are in step, and for a ring frame f its world right after LoadGameState(f) in the ring
sweep -- the oracle after Load(f) IS the frame's content.  Backend B is only ever asked; what it answered before the sweep's first Load is kept and compared at the
end of the sweep, when A has shown every frame.  Resource words are the adapter's model's (A.model.cur).  The witness knows nothing of blocks, slots or kernels.

Per session it collects `hit`: the classes of CLASSES that the models -- the oracle's states alone -- say the session showed.  tests/test_fuzz_inspect.py chooses the
committed seeds (CASES) so that the classes are met, and pins them in HIT; the GPU tier asserts that a device session hit exactly what is pinned for its seed.

Not used with start_frame sessions: the window of frames on_list asks about is plain integer arithmetic.
(A helper module, no tests of its own.)"""
import numpy as np
import pytest

import bevy_ggrs_amd as bg
import checksum_parts_common as cp
import fuzz_device_spawn as fd
import fuzz_user_worlds as fu
import fuzz_util
import query_common as qc
import state_diff_common as sd
from oracle.binding import FLAT, OracleWorld

LIVE = bg.LIVE
TOGGLED = ("Stun", "Burn", "Half", "Velocity")            # the component hosts or systems insert and remove, by family; a generic world takes its first C*
CLASSES = ("alive", "presence", "value", "same", "resource", "len", "overflow", "empty", "truncated", "many", "nobody")
ENTRIES = (64, 5)
LETTERS = "apvsrloetmn"                                   # CLASSES by their first letters: how HIT spells a set of them
TRUNC = 37                                                # rows: the cut falls inside the first 64-slot unit


def letters(hit): return "".join(LETTERS[i] for i, c in enumerate(CLASSES) if c in hit)


def _name(state): return "LIVE" if state == LIVE else f"frame {state}"


class Witness:
    """cks: None = the checksum registrations are recorded from backend A while the scenario builds it (watch()); "all" = every rollback component with all its words
    (the user-written worlds, whose A is made out of reach).  no_rollback: ids of the components outside rollback.  probe(B) -> int: sampled around every callback
    that asks B something; `probe_grew` says whether it ever grew across one (slots materialised on demand)."""

    def __init__(self, cks=None, no_rollback=(), live_every=6, probe=None):
        self.cks, self.no_rollback, self.live_every, self.probe = ([] if cks is None else cks), set(no_rollback), live_every, probe
        self.returned, self.hit, self.ready = {}, set(), False
        self.sync_lists = self.asked = self.sweeps = 0
        self.probe_grew = False
        self.cap = None                                     # what before_sweep kept
        self.memo = self._shared = None
        self.tail = []

    # ---- what the family is ---------------------------------------------------------------------------------------------------------------------------------------
    def scenario(self, sc):
        if isinstance(sc, fuzz_util.GenericScenario) and sc.no_rollback >= 0: self.no_rollback = {sc.no_rollback}
        if isinstance(sc, fuzz_util.BoxScenario) and not sc.player_rollback: self.no_rollback = {2}

    def watch(self, world):
        """Records world.checksum_component(comp, words) as the scenario registers them; returns world."""
        orig = world.checksum_component

        def checksum_component(comp, words):
            self.cks.append((int(comp), [int(k) for k in words]))
            return orig(comp, words)
        world.checksum_component = checksum_component
        return world

    def _setup(self, A):
        comps = A._comps
        self.comps, col = [], 0
        for c, (_, wb, nw) in enumerate(comps):
            if c not in self.no_rollback: self.comps.append((c, col, nw))
            col += nw                                       # (a non-rollback component's words are columns too)
        cks = [(c, list(range(nw))) for c, _, nw in self.comps] if self.cks == "all" else self.cks
        assert all(c not in self.no_rollback for c, _ in cks)
        model = getattr(A, "model", None)
        res = [(name, r, wb, list(range(len(words)))) for r, (name, wb, words) in enumerate(model.layout)] if model is not None else []
        self.specs = cp.Specs(sorted(((comps[c][0], c, [(k, comps[c][1]) for k in words]) for c, words in cks), key=lambda t: t[1]), res)
        names = {comps[c][0]: c for c, _, _ in self.comps}
        tog = next((names[nm] for nm in TOGGLED if nm in names), None)
        if tog is None: tog = next(c for c, _, _ in self.comps if comps[c][0].startswith("C"))
        by_width = {}
        for c, _, nw in self.comps: by_width.setdefault(comps[c][1], (c, nw - 1))
        fetch = [by_width[wb] for wb in sorted(by_width, reverse=True)]
        fetch = fetch[1::2] + fetch[0::2]                   # neither id order nor width order
        fetch += [(c, 0) for c, k in fetch if k > 0][:max(0, 3 - len(fetch))]      # three columns at least where the named components have the words: the
        if len(fetch) < 2:                                  # offsets and the padding between columns are part of what is compared
            fetch += [(c, nw - 1) for c, _, nw in self.comps if c != fetch[0][0]][:1]
        other = [(c, 0) for c, _, _ in self.comps if c != tog][:1]
        self.toggled = tog
        self.descs = [qc.make_desc(fetch), qc.make_desc(other, with_=[tog]), qc.make_desc(other, without=[tog]), qc.make_desc()]
        self.ready = True

    def rec_of(self, A):
        """Backend A's live world in the form the three models take."""
        if self._shared is not None and "rec" in self._shared: return self._shared["rec"]
        n = A.len
        rec = {"len": n, "alive": A.alive_mask(n), "present": {}, "words": {}, "res": {}}
        for c, _, nw in self.comps:
            rec["present"][c] = A.present_mask(c, n)
            for k in range(nw): rec["words"][(c, k)] = A.download_word(c, k, 0, n)
        rec["columns"] = rec["words"]
        model = getattr(A, "model", None)
        if model is not None: rec["res"] = {r: [int(x) for x in model.cur[r]] for r in range(len(model.layout))}
        if self._shared is not None: self._shared["rec"] = rec
        return rec

    def _m(self, key, recs, fn):
        """A model's result; witnesses that look at the same recs (memo shared, test_fuzz_inspect.py) compute it once."""
        if self.memo is None: return fn()
        k = key + tuple(id(r) for r in recs)
        if k not in self.memo: self.memo[k] = (recs, fn())
        return self.memo[k][1]

    # ---- asking B -------------------------------------------------------------------------------------------------------------------------------------------------
    def _probed(self, B, fn):
        if self.probe is None: return fn()
        before = self.probe(B); out = fn()
        self.probe_grew |= self.probe(B) > before
        return out

    def _query(self, B, state, desc, max_rows):
        self.asked += 1
        if hasattr(B, "query_bytes"): return B.query_bytes(state, desc, max_rows)      # (a numpy backend has no device buffer to fill)
        return qc.device_query(B, state, desc, max_rows)

    def _parts(self, B, state): self.asked += 1; return B.checksum_parts(state)

    def _diff(self, B, a, b, **kw): self.asked += 1; return B.diff(a, b, **kw)

    # ---- holding an answer to a model ----------------------------------------------------------------------------------------------------------------------------
    def _check_parts(self, got, rec, what, ctx):
        want = self._m(("parts",), (rec,), lambda: cp.model_parts(rec, self.specs))
        assert cp.as_model(got) == want, f"checksum_parts({what}) is not the model's over the oracle's state:\n{got}\nmodel: {want}\n{ctx}"
        if any(want["counts"][name] == 0 for name, _, _ in self.specs.components): self.hit.add("nobody")
        return want

    def _check_query(self, A, got, rec, desc, max_rows, what, ctx):
        want = self._m(("query", self.descs.index(desc), max_rows), (rec,), lambda: qc.model_of(rec, desc, max_rows))
        n_matched, n_rows, buf = got
        assert (n_matched, n_rows) == (want["n_matched"], want["n_rows"]), f"query({what}, {desc}, max_rows={max_rows}): {n_matched} matched, {n_rows} rows; " \
            f"the model over the oracle's state: {want['n_matched']}, {want['n_rows']}\n{ctx}"
        exp = qc.expected_buffer(want, qc.word_bytes_of(A, desc), max_rows, buf.size)
        if not np.array_equal(buf, exp):
            bad = np.flatnonzero(buf != exp)
            raise AssertionError(f"query({what}, {desc}, max_rows={max_rows}): the output buffer differs from the model's at {bad.size} bytes, first at {bad[:8]}: "
                                 f"{buf[bad[:8]]} vs {exp[bad[:8]]}\n{ctx}")
        if want["n_matched"] == 0: self.hit.add("empty")
        if want["n_rows"] < want["n_matched"]: self.hit.add("truncated")
        if want["n_matched"] > 64: self.hit.add("many")

    def _check_diff(self, got, rec_a, rec_b, max_entries, what, ctx, classes=True):
        want = self._m(("diff", max_entries), (rec_a, rec_b), lambda: sd.model_diff(rec_a, rec_b, self.comps, max_entries))
        assert sd.as_model(got) == want, f"diff({what}, max_entries={max_entries}) is not the model's over the oracle's states:\n{got}\nmodel: {want}\n{ctx}"
        if not classes: return
        if want["n_alive"]: self.hit.add("alive")
        if want["n_presence"]: self.hit.add("presence")
        if want["n_value"]: self.hit.add("value")
        if want["resource_diff"]: self.hit.add("resource")
        if want["len_a"] != want["len_b"]: self.hit.add("len")
        if want["n_entities"] > max_entries: self.hit.add("overflow")
        if not (want["n_entities"] or want["resource_diff"] or want["len_a"] != want["len_b"]): self.hit.add("same")

    # ---- the runner's four calls ---------------------------------------------------------------------------------------------------------------------------------
    def on_list(self, A, B, reqs, checksums, in_flight=False):
        if not self.ready: self._setup(A)
        saves = [q.frame for q in reqs if isinstance(q, bg.SaveGameState)]
        assert len(saves) == len(checksums)
        for f, c in zip(saves, checksums): self.returned[f] = int(c)
        self.tail = (self.tail + [" ".join(f"S{q.frame}" if isinstance(q, bg.SaveGameState) else f"L{q.frame}" if isinstance(q, bg.LoadGameState) else "A" for q in reqs)
                                  + ("   (enqueued)" if in_flight else "")])[-6:]
        if in_flight: return                                # B may hold uncollected lists (the calls refuse), and A is ahead of it
        self.sync_lists += 1
        ctx = f"after the last of these lists (frame {B.frame}):\n" + "\n".join(self.tail)
        self._probed(B, lambda: self._on_list(A, B, ctx))

    def _on_list(self, A, B, ctx):
        if self.sync_lists % self.live_every == 0:
            rec = self.rec_of(A)
            self._check_parts(self._parts(B, LIVE), rec, "LIVE", ctx)
            for desc in self.descs:
                for cap in (rec["len"] + 64, min(TRUNC, rec["len"] // 2)):
                    self._check_query(A, self._query(B, LIVE, desc, cap), rec, desc, cap, "LIVE", ctx)
        F = B.frame
        for f in range(F - 10, F + 2):
            if f in self.returned and B.has_snapshot(f):
                got = self._parts(B, f).checksum
                assert got == self.returned[f], f"checksum_parts({f}).checksum {got:#x} is not the Checksum its SaveGameState returned, {self.returned[f]:#x}, {ctx}"

    def before_sweep(self, A, B, frames):
        if not self.ready: self._setup(A)
        self._probed(B, lambda: self._before_sweep(A, B, list(frames)))

    def _before_sweep(self, A, B, fs):
        cap = self.cap = {"frames": fs, "recs": {LIVE: self.rec_of(A)}, "parts": [], "queries": [], "diffs": [], "same": []}
        copies = {}
        for f in fs:
            p = self._parts(B, f)
            copies[f] = B.snapshot_copy(f)
            cap["parts"].append((f, p)); cap["same"].append((f"checksum_parts of frame {f} and of its snapshot_copy", cp.as_model(p), cp.as_model(self._parts(B, copies[f]))))
            for desc in self.descs:
                for rows in (p.len + 64, min(TRUNC, p.len // 2)):
                    q = self._query(B, f, desc, rows)
                    cap["queries"].append((f, desc, rows, q))
                    qb = self._query(B, copies[f], desc, rows)
                    cap["same"].append((f"query {desc} of frame {f} and of its snapshot_copy, max_rows={rows}", (q[0], q[1], q[2].tobytes()), (qb[0], qb[1], qb[2].tobytes())))
        if not fs: return
        pairs = [(fs[i + 1], fs[i]) for i in range(len(fs) - 1)] + ([(fs[-1], fs[0])] if len(fs) >= 3 else []) + [(LIVE, fs[0])]
        pairs.append((pairs[0][1], pairs[0][0]))                                       # one pair in both orders
        for a, b in pairs:
            for me in ENTRIES: cap["diffs"].append((a, b, me, True, self._diff(B, a, b, max_entries=me)))
        a, b = pairs[0]
        cap["same"].append((f"diff({_name(a)}, {_name(b)}) with and without trust_versions", sd.as_model(self._diff(B, a, b, max_entries=64)),
                            sd.as_model(self._diff(B, a, b, max_entries=64, trust_versions=True))))
        for me in ENTRIES: cap["diffs"].append((fs[-1], fs[0], me, len(fs) > 1, self._diff(B, fs[-1], copies[fs[0]], max_entries=me)))      # (a frame against a block)
        if self.no_rollback:                                                           # the documented refusal: a live-only component against a frame
            with pytest.raises(bg.GgrsHipError, match="not registered for rollback"): B.query(fs[0], [(min(self.no_rollback), 0)], max_rows=1)

    def on_sweep_frame(self, A, B, f):
        self.cap["recs"][f] = self.rec_of(A)

    def after_sweep(self, A, B, ctx):
        cap, self.cap = self.cap, None
        recs = cap["recs"]
        self.sweeps += 1
        for what, x, y in cap["same"]: assert x == y, f"{what} differ:\n{x}\n{y}\n{ctx}"
        for f, p in cap["parts"]:
            want = self._check_parts(p, recs[f], f"frame {f}", ctx)
            assert p.checksum == self.returned[f] == want["checksum"], f"frame {f}: checksum_parts says {p.checksum:#x}, its SaveGameState returned {self.returned[f]:#x}, " \
                f"the model over the oracle's state after Load({f}) gives {want['checksum']:#x}\n{ctx}"
        for f, desc, rows, q in cap["queries"]: self._check_query(A, q, recs[f], desc, rows, f"frame {f}", ctx)
        for a, b, me, classes, d in cap["diffs"]: self._check_diff(d, recs[a], recs[b], me, f"{_name(a)}, {_name(b)}", ctx, classes)


# ---- the committed cases: family -> how it runs; (family, seed) -> what it hits ----------------------------------------------------------------------------------
def _flat(sc): return OracleWorld(sc.capacity, 8, FLAT)


RUN = {"n_lists": 30, "ring_sweep": True}
FAMILIES = {
    "particles": dict(RUN), "generic": dict(RUN, generic=True), "box": dict(RUN, box=True), "plain": dict(RUN, generic=True, variant={"plain": True}),
    "tagged_particles": dict(RUN), "tagged_generic": dict(RUN, generic=True),
    "skirmish": None, "spawn": None, "brand": None, "colony": None, "skirmish_tile": None, "brand_tile": None, "colony_tile": None}


def run_case(family, seed, make_b, witness, **kw):
    """One committed case with the FLAT oracle (or oracle adapter) as backend A and `witness` looking on; returns the log."""
    if FAMILIES[family] is not None:
        def make_a(sc): witness.scenario(sc); return witness.watch(_flat(sc))
        return fuzz_util.run(seed, make_a, make_b, witness=witness, **{**FAMILIES[family], **kw})
    witness.cks = "all"
    if family == "colony": return fd.run(seed, make_b, witness=witness, **kw)[0]
    if family == "colony_tile": return fd.run(fd.TILE[0], make_b, n=fd.TILE[1], n_lists=fd.TILE[2], witness=witness, **kw)[0]
    if family.endswith("_tile"):
        s, n, n_lists = fu.TILE[family[:-5]]
        return fu.run(family[:-5], s, make_b, n=n, n_lists=n_lists, witness=witness, **kw)[0]
    return fu.run(family, seed, make_b, witness=witness, **kw)[0]


# chosen on the CPU (test_fuzz_inspect.py holds them to its floors): the seeds of each family -- a tile family has one pinned session, its seed here is a place
# holder -- and for every case the classes of CLASSES the oracle's states show, as a string of their first letters in CLASSES order (a p v s r l o e t m n)
CASES = {"particles": (0, 4, 8, 22, 27, 29, 33, 38, 47, 58, 75, 80),
         "generic": (2, 6, 9, 10, 16, 17, 21, 23, 48, 72, 74, 99),
         "box": (7, 30, 53, 54, 62, 79),
         "plain": (7004, 7006, 7010, 7017, 7018, 7029, 7036, 7071),
         "tagged_particles": (5005, 5012, 5025, 5036),
         "tagged_generic": (5010, 5017, 5018, 5024),
         "skirmish": (0, 11, 14, 17, 18, 20, 23, 27, 33, 39),
         "spawn": (201, 203, 205, 225),
         "brand": (0, 2, 4, 11, 13, 14, 16, 21),
         "colony": (6, 7, 16, 21, 35, 55, 62, 77),
         "skirmish_tile": (0,),
         "brand_tile": (0,),
         "colony_tile": (0,)}
HIT = {("particles", 0): "sen", ("particles", 4): "pvsoet", ("particles", 8): "sen", ("particles", 22): "avsloetm", ("particles", 27): "avoetm", 
       ("particles", 29): "avsloetmn", ("particles", 33): "avsot", ("particles", 38): "sen", ("particles", 47): "avoetm", ("particles", 58): "avsoetm", 
       ("particles", 75): "avslot", ("particles", 80): "vsen", ("generic", 2): "setn", ("generic", 6): "vsoet", ("generic", 9): "setmn", 
       ("generic", 10): "avsoetmn", ("generic", 16): "setn", ("generic", 17): "avsoetn", ("generic", 21): "vet", ("generic", 23): "avsoetmn", 
       ("generic", 48): "apvsotm", ("generic", 72): "avsoetmn", ("generic", 74): "avsoetn", ("generic", 99): "sen", ("box", 7): "avet", 
       ("box", 30): "avsoetm", ("box", 53): "vsoetm", ("box", 54): "pvsen", ("box", 62): "avsoetm", ("box", 79): "pvoet", ("plain", 7004): "vot", 
       ("plain", 7006): "avsoet", ("plain", 7010): "avsoetmn", ("plain", 7017): "sen", ("plain", 7018): "apvsoetmn", ("plain", 7029): "avsoetmn", 
       ("plain", 7036): "votm", ("plain", 7071): "avsoetmn", ("tagged_particles", 5005): "apvsoetm", ("tagged_particles", 5012): "avsloetmn", 
       ("tagged_particles", 5025): "avlotm", ("tagged_particles", 5036): "asloetn", ("tagged_generic", 5010): "avoet", ("tagged_generic", 5017): "apvsoetm", 
       ("tagged_generic", 5018): "avsoetmn", ("tagged_generic", 5024): "apvoetm", ("skirmish", 0): "apvrot", ("skirmish", 11): "ren", 
       ("skirmish", 14): "pvsretn", ("skirmish", 17): "avsretn", ("skirmish", 18): "apvsrotm", ("skirmish", 20): "st", ("skirmish", 23): "apvrot", 
       ("skirmish", 27): "apvsrotm", ("skirmish", 33): "setn", ("skirmish", 39): "vsrot", ("spawn", 201): "apvsrlotm", ("spawn", 203): "avsrloetn", 
       ("spawn", 205): "apvrlotm", ("spawn", 225): "apvsrotm", ("brand", 0): "apvot", ("brand", 2): "sen", ("brand", 4): "apvot", ("brand", 11): "avsetn", 
       ("brand", 13): "apvsotm", ("brand", 14): "avsetn", ("brand", 16): "apvsot", ("brand", 21): "apvsotm", ("colony", 6): "asletn", ("colony", 7): "avsetn", 
       ("colony", 16): "avlotm", ("colony", 21): "avloet", ("colony", 35): "avlotm", ("colony", 55): "avslotm", ("colony", 62): "avlot", 
       ("colony", 77): "avloetm", ("skirmish_tile", 0): "apvsroetmn", ("brand_tile", 0): "apvotm", ("colony_tile", 0): "avslotm"}
