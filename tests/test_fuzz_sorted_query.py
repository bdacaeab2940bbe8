"""CPU tier of the sorted-query witness (tests/sorted_query_witness.py), so that the GPU tier (test_gpu_zfuzz_sorted_query.py) cannot go hollow.  Every committed
(family, seed) runs once here with the FLAT oracle (adapter) as backend A and, as backend B behind enqueue / collect, the ShadowInspector of test_fuzz_inspect.py
-- the REFSHAPED oracle walked request by request, a rec kept at every Save -- with a view that also serves World.query_sorted from
sorted_query_common.model_query_sorted over those recs:

  * plumbing: the witness passes on it in every session, on every held frame before the sweep and on LIVE in mid-session;
  * coverage floors, from the oracle's recs alone: every class of sorted_query_witness.CLASSES is hit by the committed seeds as FLOORS says, and every session
    hits exactly what sorted_query_witness.HIT pins for it."""
import pytest

import bevy_ggrs_amd as bg
import inspect_witness as iw
import query_common as qc
import sorted_query_common as sq
import sorted_query_witness as sw
import test_fuzz_inspect as tfi                                                      # (the module, not its tests: ShadowInspector, View, Teeth, make_shadow)

LIVE = bg.LIVE
# how many of the 16 committed sessions must show each class
# (a generic world has no 8-byte word and a colony's first key does not tie: 12 of 16 at the most for wide8 and two_keys; the large form needs a result beyond 2048
# rows, which only the generic family's larger worlds have)
FLOORS = {"ties": 6, "desc": 14, "two_keys": 8, "wide8": 8, "float_neg": 14, "truncated": 14, "empty": 4, "small_form": 16, "large_form": 2}


class SortedView(tfi.View):
    """The shadow's inspection surface with World.query_sorted."""

    def __init__(self, shadow): super().__init__(shadow, None)

    def query_sorted_bytes(self, state, desc, order_by, max_rows, extra=512):
        rec = self._rec(state)
        wbs = qc.word_bytes_of(self.sh, desc)
        m = self._m(("sorted", repr(sorted(desc.items(), key=str)), repr(order_by), max_rows), (rec,), lambda: sq.model_query_sorted(rec, desc, order_by, max_rows))
        return m["n_matched"], m["n_rows"], sq.expected_buffer(m, wbs, max_rows, qc.model_layout(wbs, desc["slots"], max_rows)[2] + extra)


class Teeth(tfi.Teeth):
    """tfi.Teeth over one sorted-query witness and the true view."""

    def __init__(self):
        self.cfg = iw.Witness()
        self.inner = {None: sw.SortedWitness()}
        self.memo, self.failed, self.views = {}, {}, None
        for w in self.inner.values(): w.memo = self.memo

    def shadow(self, world):
        sh = tfi.ShadowInspector(world, self.cfg)
        self.views = {None: SortedView(sh)}
        return sh


_SESSIONS = {}


def session(family, seed):
    """One case, run once and shared: {"log", "hit": the classes as sorted_query_witness.HIT spells them}."""
    key = (family, seed)
    if key not in _SESSIONS:
        t = Teeth()
        log = sw.run_case(family, seed, tfi.make_shadow(family, t), t)
        w = t.inner[None]
        assert w.sweeps == 2 and w.sync_lists >= 1 and w.asked > 20, (log[0], w.sweeps, w.sync_lists, w.asked)
        _SESSIONS[key] = {"log": log, "hit": sw.letters(t.hit)}
    return _SESSIONS[key]


ALL_CASES = [(f, s) for f, seeds in sw.CASES.items() for s in seeds]


@pytest.mark.parametrize("family,seed", ALL_CASES, ids=[f"{f}-{s}" for f, s in ALL_CASES])
def test_the_witness_passes_on_the_shadow_and_hits_what_is_pinned(family, seed):
    s = session(family, seed)
    assert s["hit"] == sw.HIT[family, seed], (s["log"][0], s["hit"])


def test_coverage_floors_of_the_committed_seeds():
    ss = [session(f, s) for f, s in ALL_CASES]
    for c, floor in FLOORS.items():
        n = sum(sw.LETTERS[sw.CLASSES.index(c)] in s["hit"] for s in ss)
        print(f"{c} in {n}/{len(ss)} sessions")
        assert n >= floor, (c, n, floor)
    assert set(FLOORS) == set(sw.CLASSES) and set(sw.HIT) == set(ALL_CASES)
    for f in ("particles", "generic", "skirmish", "colony"): assert len(sw.CASES[f]) == 4 and all(s in iw.CASES[f] for s in sw.CASES[f]), f


def test_the_library_has_the_entry_point():
    assert callable(getattr(bg.World, "query_sorted"))                                # (on the parent the witness has nothing to ask)
