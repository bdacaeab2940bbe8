"""CPU tier of the delta witness (tests/delta_witness.py), so that the GPU tier (test_gpu_zfuzz_delta.py) cannot go hollow.  Every committed (family, seed) runs
once here with the FLAT oracle (adapter) as backend A and, as backend B behind enqueue / collect, the ShadowInspector of test_fuzz_inspect.py -- the REFSHAPED
oracle walked request by request, a rec kept at every Save -- with a view that also serves World.delta from delta_common.model_delta over those recs:

  * plumbing: the witness passes on it in every session -- also the answers it asked for in mid-session and judged a sweep later, which holds its premise that a
    ring frame changes by a Save alone;
  * teeth: the same session is shown to the three wrong models of delta_common.WRONG, each through a witness of its own; the two that get the alive bits wrong
    are caught in every family, the one that compares absent components (RARE) where the oracle's states can show it;
  * coverage floors, from the oracle's recs alone: in each family every kind returns a non-empty result and a CHANGED result is a strict, non-empty subset of the
    live entities; some session has rows beyond old's len; and every session hits exactly what delta_witness.HIT pins for it."""
import pytest

import bevy_ggrs_amd as bg
import delta_common as dc
import delta_witness as dw
import inspect_witness as iw
import query_common as qc
import test_fuzz_inspect as tfi                                                      # (the module, not its tests: ShadowInspector, View, Teeth, make_shadow)

LIVE = bg.LIVE
FLOOR = ("changed", "added", "removed", "despawned", "subset")
GROUPS = ("particles", "generic", "box", "plain", "tagged", "skirmish", "colony")
# a component absent on both sides of two held states, over bytes that differ, in an entity alive on both: of the sessions of inspect_witness.CASES in these
# families only colony 77 and the tile sessions show it; the hand-written cases of test_delta_model.py and the scenes of test_gpu_delta.py hold it everywhere
RARE = "absent_on_both_sides_is_changed"


class DeltaView(tfi.View):
    """The shadow's inspection surface with World.delta; `bug`: the wrong model it answers from (delta_common.WRONG), or None."""

    def __init__(self, shadow, bug): super().__init__(shadow, None); self.bug = bug

    def delta_bytes(self, new, old, desc, max_rows, extra=512):
        rec_new, rec_old = self._rec(new), self._rec(old)
        model = dc.model_delta if self.bug is None else dc.wrong_model(self.bug)
        wbs = dc.word_bytes_of(self.sh, desc)
        m = self._m(("delta", self.bug, repr(sorted(desc.items(), key=str)), max_rows), (rec_new, rec_old), lambda: model(rec_new, rec_old, desc, max_rows))
        buf = qc.expected_buffer(m, wbs, max_rows, qc.model_layout(wbs, desc["q"]["slots"], max_rows)[2] + extra)
        return (m["n_matched"], m["n_rows"], m["n_beyond_old_len"], m["len_new"], m["len_old"]), buf

    def delta(self, new, old, fetch=(), *, kind="changed", changed=(), **kw):
        named = set(changed) & self.sh.cfg.no_rollback
        if named and not (new == LIVE and old == LIVE): raise bg.GgrsHipError(-1, f"changed_mask names component {min(named)}, which is not registered for rollback")
        raise NotImplementedError("the shadow serves whole buffers: delta_bytes")


class Teeth(tfi.Teeth):
    """tfi.Teeth over delta witnesses: the true view and one per wrong model."""

    def __init__(self):
        self.cfg = iw.Witness()
        self.inner = {name: dw.DeltaWitness() for name in (None,) + dc.WRONG}
        self.memo, self.failed, self.views = {}, {}, None
        for w in self.inner.values(): w.memo = self.memo

    def shadow(self, world):
        sh = tfi.ShadowInspector(world, self.cfg)
        self.views = {name: DeltaView(sh, name) for name in self.inner}
        return sh


_SESSIONS = {}


def session(family, seed):
    """One case, run once and shared: {"log", "hit": the classes as delta_witness.HIT spells them, "failed": wrong model -> its witness's first complaint}."""
    key = (family, seed)
    if key not in _SESSIONS:
        t = Teeth()
        log = dw.run_case(family, seed, tfi.make_shadow(family, t), t)
        w = t.inner[None]
        assert w.sweeps == 2 and w.sync_lists >= 1 and w.asked > 20, (log[0], w.sweeps, w.sync_lists, w.asked)
        _SESSIONS[key] = {"log": log, "hit": dw.letters(t.hit), "failed": dict(t.failed)}
    return _SESSIONS[key]


ALL_CASES = [(f, s) for f, seeds in dw.CASES.items() for s in seeds]


@pytest.mark.parametrize("family,seed", ALL_CASES, ids=[f"{f}-{s}" for f, s in ALL_CASES])
def test_the_witness_passes_on_the_shadow_and_hits_what_is_pinned(family, seed):
    s = session(family, seed)
    assert s["hit"] == dw.HIT[family, seed], (s["log"][0], s["hit"])


def _by_group():
    out = {}
    for f, s in ALL_CASES: out.setdefault(tfi.group(f), []).append(session(f, s))
    return out


def test_every_wrong_model_is_caught_in_every_family():
    by = _by_group()
    assert set(by) == set(GROUPS)
    for g, ss in by.items():
        for bug in dc.WRONG:
            caught = sum(bug in s["failed"] for s in ss)
            print(f"{bug} in {g}: caught in {caught}/{len(ss)} sessions")
            if bug != RARE: assert caught >= 2, (bug, g)
    assert sum(RARE in s["failed"] for ss in by.values() for s in ss) >= 2


def test_coverage_floors_of_the_committed_seeds():
    by = _by_group()
    for g, ss in by.items():
        for c in FLOOR:
            n = sum(dw.LETTERS[dw.CLASSES.index(c)] in s["hit"] for s in ss)
            print(f"{g}: {c} in {n}/{len(ss)} sessions")
            assert n >= 1, (g, c)
    assert any("b" in s["hit"] for ss in by.values() for s in ss)                    # rows beyond old's len: somebody must spawn before it can insert
    assert sum(f.endswith("_tile") for f in dw.CASES) == 2 and set(dw.HIT) == set(ALL_CASES) and all(s in iw.CASES[f] for f, s in ALL_CASES)
