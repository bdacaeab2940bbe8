"""A witness for the request fuzzers (fuzz_util.run(witness=...)): World.delta asked about the ring frames and the live world of random sessions, all four kinds,
and held to delta_common.model_delta over what the ORACLE says those states are.  Built on inspect_witness.Witness: what the family is, the oracle's recs (rec_of),
the runner's four calls and their order are its; only what is asked and what it is held to differ.

    after a list that is not in flight   every kind on LIVE against LIVE (the model over the oracle's live world: nothing differs), every live_every-th list;
                                         every kind on the two newest frames held near the current one -- a mid-session reader of owed ring slots.  Those answers
                                         are kept and judged in the next sweep, if neither frame was saved again until then (a slot changes by a Save alone)
    before a ring sweep                  every kind on adjacent held frames, oldest against newest in both orders, LIVE against the newest, every frame against its
                                         snapshot_copy (nothing differs) and the newest against the oldest one's copy (what the frame itself gave); kept, and judged
                                         when the sweep has shown the oracle's state of every frame

`hit`: the classes of CLASSES the models -- the oracle's states alone -- say the session showed.  tests/test_fuzz_delta.py chooses the committed seeds (CASES) so
that its floors are met and pins them in HIT; the GPU tier asserts that a device session hit exactly what is pinned.
(A helper module, no tests of its own.)"""
import numpy as np

import bevy_ggrs_amd as bg
import delta_common as dc
import inspect_witness as iw
import query_common as qc

LIVE = bg.LIVE
CLASSES = ("changed", "added", "removed", "despawned", "subset", "beyond", "truncated")          # a kind: a non-empty result of it; subset: a CHANGED result that is
LETTERS = "cardsbt"                                                                                # a strict, non-empty subset of new's live entities; beyond: n_beyond_old_len > 0
TRUNC = iw.TRUNC


def letters(hit): return "".join(LETTERS[i] for i, c in enumerate(CLASSES) if c in hit)


class DeltaWitness(iw.Witness):
    def _setup(self, A):
        super()._setup(A)
        every = [c for c, _, _ in self.comps]
        tog = self.toggled
        wide, other = self.descs[0]["fetch"], self.descs[1]["fetch"]
        quiet = [c for c in every if c != tog][-1:] or every[:1]
        self.ddescs = [dc.make_delta("changed", every, wide), dc.make_delta("changed", quiet, other, without=[tog]), dc.make_delta("changed", [tog], []),
                       dc.make_delta("added", [tog] + quiet, other), dc.make_delta("removed", every, other), dc.make_delta("removed", [tog], [], slots=True),
                       dc.make_delta("despawned", (), wide), dc.make_delta("despawned", (), [], without=[tog])]
        self.save_count, self.kept = {}, []

    # ---- asking B, holding an answer to the model -----------------------------------------------------------------------------------------------------------------
    def _delta(self, B, new, old, desc, max_rows):
        self.asked += 1
        if hasattr(B, "delta_bytes"): return B.delta_bytes(new, old, desc, max_rows)                # (a numpy backend has no device buffer to fill)
        return dc.device_delta(B, new, old, desc, max_rows)

    def _ask_all(self, B, new, old, len_hint):
        return [(desc, cap, self._delta(B, new, old, desc, cap)) for desc in self.ddescs for cap in (len_hint + 64, min(TRUNC, len_hint // 2))]

    def _check_delta(self, A, got, rec_new, rec_old, desc, max_rows, what, ctx, classes=True):
        want = self._m(("delta", self.ddescs.index(desc), max_rows), (rec_new, rec_old), lambda: dc.model_delta(rec_new, rec_old, desc, max_rows))
        rep, buf = got
        exp_rep = (want["n_matched"], want["n_rows"], want["n_beyond_old_len"], want["len_new"], want["len_old"])
        assert tuple(rep) == exp_rep, f"delta({what}, {desc}, max_rows={max_rows}) reports {tuple(rep)}; the model over the oracle's states: {exp_rep}\n{ctx}"
        exp = qc.expected_buffer(want, dc.word_bytes_of(A, desc), max_rows, buf.size)
        if not np.array_equal(buf, exp):
            bad = np.flatnonzero(buf != exp)
            raise AssertionError(f"delta({what}, {desc}, max_rows={max_rows}): the output buffer differs from the model's at {bad.size} bytes, first at {bad[:8]}: "
                                 f"{buf[bad[:8]]} vs {exp[bad[:8]]}\n{ctx}")
        if not classes: return
        if want["n_matched"]: self.hit.add(desc["kind"])
        if want["n_beyond_old_len"]: self.hit.add("beyond")
        if want["n_rows"] < want["n_matched"]: self.hit.add("truncated")
        if desc["kind"] == "changed" and 0 < want["n_matched"] < int(qc.as_bits(rec_new["alive"], rec_new["len"]).sum()): self.hit.add("subset")

    # ---- the runner's four calls ----------------------------------------------------------------------------------------------------------------------------------
    def on_list(self, A, B, reqs, checksums, in_flight=False):
        if not self.ready: self._setup(A)
        for q in reqs:
            if isinstance(q, bg.SaveGameState): self.save_count[q.frame] = self.save_count.get(q.frame, 0) + 1
        super().on_list(A, B, reqs, checksums, in_flight=in_flight)

    def _on_list(self, A, B, ctx):
        if self.sync_lists % self.live_every == 0:
            rec = self.rec_of(A)
            for desc, cap, got in self._ask_all(B, LIVE, LIVE, rec["len"]): self._check_delta(A, got, rec, rec, desc, cap, "LIVE, LIVE", ctx, classes=False)
        F = B.frame
        held = [f for f in range(F + 1, F - 10, -1) if f in self.returned and B.has_snapshot(f)][:2]
        if len(held) == 2:
            new, old = held
            self.kept = self.kept[-2:] + [(new, old, (self.save_count.get(new), self.save_count.get(old)), self._ask_all(B, new, old, A.len), ctx)]

    def _before_sweep(self, A, B, fs):
        cap = self.cap = {"frames": fs, "recs": {LIVE: self.rec_of(A)}, "asks": [], "same": []}
        if not fs: return
        n = cap["recs"][LIVE]["len"]
        pairs = [(fs[i], fs[i + 1]) for i in range(len(fs) - 1)] + [(fs[0], fs[-1]), (fs[-1], fs[0]), (LIVE, fs[0])]
        for new, old in pairs: cap["asks"].append((new, old, old, self._ask_all(B, new, old, n)))
        copies = {f: B.snapshot_copy(f) for f in fs}
        for f in fs: cap["asks"].append((f, f, copies[f], self._ask_all(B, f, copies[f], n)))
        via_block = self._ask_all(B, fs[0], copies[fs[-1]], n)
        for (desc, rows, x), (_, _, y) in zip(cap["asks"][len(fs) - 1][3], via_block):
            cap["same"].append((f"delta {desc} of frame {fs[0]} against frame {fs[-1]} and against its snapshot_copy, max_rows={rows}", (x[0], x[1].tobytes()), (y[0], y[1].tobytes())))
        if self.no_rollback:                                                           # the documented refusal: a live-only component against a frame
            import pytest
            with pytest.raises(bg.GgrsHipError, match="not registered for rollback"): B.delta(fs[0], fs[0], kind="added", changed=[min(self.no_rollback)], max_rows=0)

    def after_sweep(self, A, B, ctx):
        cap, self.cap = self.cap, None
        kept, self.kept = self.kept, []
        recs = cap["recs"]
        self.sweeps += 1
        for what, x, y in cap["same"]: assert x == y, f"{what} differ\n{ctx}"
        for new, old, _, answers in cap["asks"]:
            for desc, rows, got in answers: self._check_delta(A, got, recs[new], recs[old], desc, rows, f"{iw._name(new)}, {iw._name(old)}", ctx)
        for new, old, counts, answers, then in kept:                                   # asked in mid-session: the frames are what they were iff nobody saved them again
            if new in recs and old in recs and new != LIVE and counts == (self.save_count.get(new), self.save_count.get(old)):
                for desc, rows, got in answers: self._check_delta(A, got, recs[new], recs[old], desc, rows, f"frame {new}, frame {old} (asked in mid-session)", then + "\n" + ctx)


def run_case(family, seed, make_b, witness, **kw): return iw.run_case(family, seed, make_b, witness, **kw)


# chosen on the CPU (test_fuzz_delta.py holds them to its floors): the seeds of each family, all of them among inspect_witness.CASES, and for every case the classes
# of CLASSES the oracle's states show, as a string of their first letters in LETTERS order (c a r d s b t)
CASES = {"particles": (4, 22, 47, 75),
         "generic": (6, 10, 23, 48),
         "box": (7, 30, 62),
         "plain": (7006, 7010, 7018, 7071),
         "tagged_particles": (5005, 5025),
         "tagged_generic": (5017, 5024),
         "skirmish": (0, 17, 18, 23),
         "colony": (7, 16, 35, 77),
         "skirmish_tile": (0,),
         "colony_tile": (0,)}
HIT = {("particles", 4): "carst", ("particles", 22): "cardbt", ("particles", 47): "cardst", ("particles", 75): "cardsbt", ("generic", 6): "cst",
       ("generic", 10): "cardst", ("generic", 23): "cardst", ("generic", 48): "cardst", ("box", 7): "crds", ("box", 30): "cardst",
       ("box", 62): "cardst", ("plain", 7006): "cardst", ("plain", 7010): "cardst", ("plain", 7018): "cardst", ("plain", 7071): "cardst",
       ("tagged_particles", 5005): "cardst", ("tagged_particles", 5025): "cardsbt", ("tagged_generic", 5017): "cardst", ("tagged_generic", 5024): "cardst", ("skirmish", 0): "crds",
       ("skirmish", 17): "cardst", ("skirmish", 18): "cardst", ("skirmish", 23): "cardst", ("colony", 7): "cardt", ("colony", 16): "cardsbt",
       ("colony", 35): "cardsbt", ("colony", 77): "cardsbt", ("skirmish_tile", 0): "cardst", ("colony_tile", 0): "cardsbt"}
