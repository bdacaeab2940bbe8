"""A witness for the request fuzzers (fuzz_util.run(witness=...)): World.query_sorted asked about the ring frames and the live world of random sessions, ordered
by the worlds' own columns, and held to sorted_query_common.model_query_sorted over what the ORACLE says those states are.  Built on inspect_witness.Witness: what
the family is, the oracle's recs (rec_of), the runner's four calls and their order are its; only what is asked and what it is held to differ.

The orders, from the world's own rollback components (particles: Transform / Velocity are f32 words, Ttl is the u64):
    pos      the first 4-byte word of the world, as an f32 (GGRS_SORT_F), ascending; the wide fetch
    wide     the first 8-byte word descending, then pos (a world without an 8-byte word: its last word as an integer, descending, then pos)
    toggled  word 0 of the component hosts or systems insert and remove (an implied With that changes between frames), by itself; slots only

    after a list that is not in flight   every order on LIVE, every live_every-th list, held at once to the model over the oracle's live world
    before a ring sweep                  every order on every held frame; kept, and judged when the sweep has shown the oracle's state of every frame
each once with max_rows = len + 64 and once cut at min(TRUNC, len // 2).  A device backend answers every question in both forms (one workgroup in one launch
where the result fits it, and the radix launches forced): the two buffers must be the same bytes.

`hit`: the classes of CLASSES the models -- the oracle's states alone -- say the session showed.  tests/test_fuzz_sorted_query.py chooses the committed seeds
(CASES) so that its floors are met and pins them in HIT; the GPU tier asserts that a device session hit exactly what is pinned.
(A helper module, no tests of its own.)"""
import numpy as np

import bevy_ggrs_amd as bg
import inspect_witness as iw
import query_common as qc
import sorted_query_common as sq

LIVE = bg.LIVE
# ties: two matched rows equal on every key (the slot decides); desc: a descending key over more than one row; two_keys: the first key ties among the matched rows,
# so a later key decides; wide8: an 8-byte key over more than one row; float_neg: an F key whose sign bit is set in a matched row; small_form / large_form: a
# non-empty result of at most / more than SMALL_MAX rows (the form the library takes by size)
CLASSES = ("ties", "desc", "two_keys", "wide8", "float_neg", "truncated", "empty", "small_form", "large_form")
LETTERS = "tdkwfcesl"
TRUNC = iw.TRUNC
SMALL_MAX = 2048


def letters(hit): return "".join(LETTERS[i] for i, c in enumerate(CLASSES) if c in hit)


class SortedWitness(iw.Witness):
    def _setup(self, A):
        super()._setup(A)
        wb_of = {c: A._comps[c][1] for c, _, _ in self.comps}
        tog = self.toggled
        four = [c for c, _, _ in self.comps if wb_of[c] == 4]
        eight = [c for c, _, _ in self.comps if wb_of[c] == 8]
        pos = (four[0], 0, "f") if four else (self.comps[0][0], 0, "u")
        last = self.comps[-1]
        wide = (eight[0], 0, "u", "desc") if eight else (last[0], last[2] - 1, "i", "desc")
        other = self.descs[1]["fetch"]
        self.asks_of = [(self.descs[0], [pos]), (qc.make_desc(other), [wide, pos]), (qc.make_desc([]), [(tog, 0, "f" if wb_of[tog] >= 4 else "i")])]
        self.wb_of = wb_of

    # ---- asking B, holding an answer to the model -----------------------------------------------------------------------------------------------------------------
    def _sorted(self, B, state, desc, order_by, max_rows):
        self.asked += 1
        if hasattr(B, "query_sorted_bytes"): return B.query_sorted_bytes(state, desc, order_by, max_rows)      # (a numpy backend has no device buffer to fill)
        try:
            assert B._lib.ggrs_dbg_set_sort_form(B._p, 1) == 0
            large = sq.device_query_sorted(B, state, desc, order_by, max_rows)
        finally:
            B._lib.ggrs_dbg_set_sort_form(B._p, 0)
        got = sq.device_query_sorted(B, state, desc, order_by, max_rows)
        assert got[:2] == large[:2] and np.array_equal(got[2], large[2]), f"query_sorted({iw._name(state)}, {desc}, {order_by}, max_rows={max_rows}): the two forms wrote different bytes"
        return got

    def _ask_all(self, B, state, len_hint):
        return [(k, cap, self._sorted(B, state, desc, order_by, cap)) for k, (desc, order_by) in enumerate(self.asks_of) for cap in (len_hint + 64, min(TRUNC, len_hint // 2))]

    def _check_sorted(self, A, got, rec, k, max_rows, what, ctx):
        desc, order_by = self.asks_of[k]
        want = self._m(("sorted", k, max_rows), (rec,), lambda: sq.model_query_sorted(rec, desc, order_by, max_rows))
        n_matched, n_rows, buf = got
        assert (n_matched, n_rows) == (want["n_matched"], want["n_rows"]), f"query_sorted({what}, {desc}, {order_by}, max_rows={max_rows}): {n_matched} matched, {n_rows} rows; " \
            f"the model over the oracle's state: {want['n_matched']}, {want['n_rows']}\n{ctx}"
        exp = sq.expected_buffer(want, qc.word_bytes_of(A, desc), max_rows, buf.size)
        if not np.array_equal(buf, exp):
            bad = np.flatnonzero(buf != exp)
            raise AssertionError(f"query_sorted({what}, {desc}, {order_by}, max_rows={max_rows}): the output buffer differs from the model's at {bad.size} bytes, first at {bad[:8]}: "
                                 f"{buf[bad[:8]]} vs {exp[bad[:8]]}\n{ctx}")
        self.hit |= self._m(("sorted classes", k, max_rows), (rec,), lambda: classes_of(rec, desc, order_by, max_rows, want))

    # ---- the runner's four calls ----------------------------------------------------------------------------------------------------------------------------------
    def _on_list(self, A, B, ctx):
        if self.sync_lists % self.live_every == 0:
            rec = self.rec_of(A)
            for k, cap, got in self._ask_all(B, LIVE, rec["len"]): self._check_sorted(A, got, rec, k, cap, "LIVE", ctx)

    def _before_sweep(self, A, B, fs):
        self.cap = {"frames": fs, "recs": {LIVE: self.rec_of(A)}, "asks": [(f, self._ask_all(B, f, A.len)) for f in fs]}

    def after_sweep(self, A, B, ctx):
        cap, self.cap = self.cap, None
        self.sweeps += 1
        for f, answers in cap["asks"]:
            for k, rows, got in answers: self._check_sorted(A, got, cap["recs"][f], k, rows, f"frame {f}", ctx)


def classes_of(rec, desc, order_by, max_rows, want):
    """What one answer shows, from the model's inputs alone."""
    hit = set()
    keys = [sq.norm_key(k) for k in order_by]
    everyone = sq.model_query_sorted(rec, qc.make_desc(desc["fetch"], desc["with"], desc["without"]), order_by, rec["len"])["slots"].astype(np.int64)
    n = want["n_matched"]
    assert everyone.size == n
    if n == 0: hit.add("empty")
    elif n <= SMALL_MAX: hit.add("small_form")
    else: hit.add("large_form")
    if want["n_rows"] < n: hit.add("truncated")
    if n > 1:
        cols = [np.asarray(rec["columns"][(c, w)])[everyone] for c, w, _, _ in keys]
        images = np.stack([sq.key_image(col, col.dtype.itemsize, kind, dsc) for col, (_, _, kind, dsc) in zip(cols, keys)], axis=1)
        if np.unique(images, axis=0).shape[0] < n: hit.add("ties")
        if any(dsc for _, _, _, dsc in keys): hit.add("desc")
        if len(keys) >= 2 and np.unique(images[:, 0]).size < n: hit.add("two_keys")
        if any(col.dtype.itemsize == 8 for col in cols): hit.add("wide8")
    for (c, w, kind, _) in keys:
        if kind == "f" and n:
            col = np.asarray(rec["columns"][(c, w)])[everyone]
            if (col >> (8 * col.dtype.itemsize - 1)).any(): hit.add("float_neg")
    return hit


def run_case(family, seed, make_b, witness, **kw): return iw.run_case(family, seed, make_b, witness, **kw)


# chosen on the CPU (test_fuzz_sorted_query.py holds them to its floors): four sessions each of particles, generic, skirmish and the colony, all of them among
# inspect_witness.CASES (two of the generic ones have results longer than one sort tile); for every case the classes of CLASSES the oracle's states show, as a
# string of their first letters in LETTERS order (t d k w f c e s l)
CASES = {"particles": (22, 29, 47, 75), "generic": (9, 23, 48, 72), "skirmish": (0, 17, 18, 23), "colony": (6, 16, 35, 55)}
HIT = {("particles", 22): "tdkwfcs", ("particles", 29): "tdkwfces", ("particles", 47): "dkwfcs", ("particles", 75): "tdkwfcs",
       ("generic", 9): "dkfcesl", ("generic", 23): "dkfces", ("generic", 48): "dkfcsl", ("generic", 72): "dkfces",
       ("skirmish", 0): "tdkwfcs", ("skirmish", 17): "dkwfces", ("skirmish", 18): "tdkwfcs", ("skirmish", 23): "tdkwfcs",
       ("colony", 6): "dwfces", ("colony", 16): "dwfcs", ("colony", 35): "tdwfcs", ("colony", 55): "tdwfcs"}
