"""CPU tier of the inspection witness (tests/inspect_witness.py), so that the GPU tier (test_gpu_zfuzz_inspect.py) cannot go hollow.  Every committed (family, seed)
runs ONCE here, with the FLAT oracle (adapter) as backend A and, as backend B behind enqueue / collect -- the stream the HIP backend gets --, a ShadowInspector:

  * plumbing: the ShadowInspector wraps the REFSHAPED oracle (adapter), walks every list request by request, keeps a rec at every Save and serves checksum_parts /
    diff / query / snapshot_copy from the three numpy models over those recs.  The witness passes on it in every session: the runner's four calls come in the order
    the witness needs, and the premise holds that the oracle's world after Load(f) is what the last Save(f) held -- to the bit, the Checksum the Save returned
    included (which also pins the Specs the witness builds from the registrations);
  * teeth: beside the true inspector the same session is shown to five deliberately wrong ones (WRONG), each through a witness of its own; each must make its
    witness fail in three sessions at least of every family that can show it (TEETH);
  * coverage floors: from the oracle's recs alone (Witness.hit), in each family three sessions at least hold each class of FLOORS; and every session hits exactly
    the classes pinned for it in inspect_witness.HIT, which is what the GPU tier holds a device session to.

Classes left out of FLOORS for a family, that family only:
  * "resource", a held pair whose resource words differ: only the skirmish worlds have device resources;
  * "len", a held pair whose lens differ: only worlds that spawn -- particles with spawn, skirmish with host spawns, colony;
  * "presence", a held pair with a presence difference, in the worlds where only the HOST inserts and removes (particles, generic, box_game, plain): most lists open
    with a Load, which takes the edit back, so that two held frames straddle one in 1 session of 100 (particles 0..99, generic 0..99, plain 7000..7079) or 2 of 80
    (box_game); the one seed that shows it is among the committed ones.  The tagged worlds reach it in 3 of 100 (all three are committed), and the LIVE checks and
    the "presence" inspector below cover presence in every family;
  * "nobody", a checksummed component held by nobody, in box_game (2 sessions of 80: every cube has every component, so it takes a world that died out) and in
    the colony (2 of the 25 seeds of fuzz_device_spawn.SEEDS);
  * "empty" and "nobody" in the skirmish with host spawns: both take a world of one or two, "many" takes one of more than 64, and the family has four sessions.
    No four of the seeds 200..229 hold three of each; the committed four hold "empty" and "nobody" once."""
import numpy as np
import pytest

import bevy_ggrs_amd as bg
import checksum_parts_common as cp
import fuzz_device_spawn as fd
import fuzz_user_worlds as fu
import fuzz_util
import inspect_witness as iw
import query_common as qc
import state_diff_common as sd
from bevy_ggrs_amd.world import ChecksumParts, DiffEntry, StateDiff
from oracle.binding import REFSHAPED, OracleWorld
from test_fuzz_requests import InFlight

LIVE = bg.LIVE
WRONG = ("len", "dead", "first", "res", "presence")
_ALL = ("particles", "generic", "box", "plain", "tagged", "skirmish", "spawn", "brand", "colony")
TEETH = {"len": ("particles", "spawn", "colony"), "dead": _ALL, "first": _ALL, "res": ("skirmish", "spawn"), "presence": _ALL}
_BASE = ("alive", "value", "same", "overflow", "empty", "truncated", "many")
FLOORS = {"particles": _BASE + ("len", "nobody"), "generic": _BASE + ("nobody",), "box": _BASE, "plain": _BASE + ("nobody",), "tagged": _BASE + ("presence", "nobody"),
          "skirmish": _BASE + ("presence", "resource", "nobody"), "spawn": ("alive", "presence", "value", "same", "resource", "len", "overflow", "truncated", "many"),
          "brand": _BASE + ("presence", "nobody"), "colony": _BASE + ("len",)}


def group(family):
    """The family a case counts under: the tile sessions with their worlds, the two tagged families as one."""
    return {"skirmish_tile": "skirmish", "brand_tile": "brand", "colony_tile": "colony", "tagged_particles": "tagged", "tagged_generic": "tagged"}.get(family, family)


# ---- the shadow inspector ----------------------------------------------------------------------------------------------------------------------------------------
def _fit(a, n):
    a = np.asarray(a)
    return a[:n] if a.size >= n else np.concatenate([a, np.zeros(n - a.size, dtype=a.dtype)])


class Block:
    """What a shadow's snapshot_copy hands out: the rec it served for that frame."""
    def __init__(self, rec): self.rec = rec


class ShadowInspector:
    """An oracle world (or adapter) that also answers the inspection calls, from the numpy models over the recs it took at every Save.  `cfg`: a Witness of the same
    family, for what the family is (rollback components, Specs) and for rec_of."""

    def __init__(self, world, cfg): self.__dict__.update(_w=world, cfg=cfg, recs={}, first={}, prev_res={}, last_res=None, gen=0, memo={})

    def __getattr__(self, k): return getattr(self._w, k)

    def handle_requests(self, reqs):
        w, out = self._w, []
        if not self.cfg.ready: self.cfg._setup(w)
        self.__dict__["gen"] += 1
        for r in reqs:
            out += w.handle_requests([r])
            if isinstance(r, bg.SaveGameState):
                rec = self.cfg.rec_of(w)
                self.first.setdefault(r.frame, rec)
                self.recs[r.frame] = rec
                self.prev_res[r.frame] = self.last_res if self.last_res is not None else rec["res"]
                self.__dict__["last_res"] = rec["res"]
        return out

    def view(self, wrong=None): return View(self, wrong)


class View:
    """The inspection surface of a ShadowInspector; `wrong` names the one thing it gets deliberately wrong:
         len        ignores len: hashes, matches and compares the slots at or beyond it (they hold what a longer timeline left there)
         dead       counts dead slots' words
         first      serves a frame's first Save of the session where it was saved twice (a slot that was not written again)
         res        serves the resource words as of the previous Save
         presence   takes presence from the live world instead of the frame"""

    def __init__(self, shadow, wrong): self.sh, self.wrong, self.cache = shadow, wrong, {}

    frame = property(lambda self: self.sh.frame)
    len = property(lambda self: self.sh.len)
    _comps = property(lambda self: self.sh._comps)

    def has_snapshot(self, f): return self.sh.has_snapshot(f)

    def _live(self):
        key = ("live", self.sh.gen)
        if key not in self.sh.memo: self.sh.memo[key] = self.sh.cfg.rec_of(self.sh._w)
        return self.sh.memo[key]

    def _rec(self, state):
        if isinstance(state, Block): return state.rec
        sh = self.sh
        if state == LIVE: base = self._live()
        else:
            if not sh.has_snapshot(state): raise bg.GgrsHipError(-1, f"frame {state} is not in the ring")
            base = sh.first[state] if self.wrong == "first" else sh.recs[state]
        if self.wrong in (None, "first"): return base
        key = (id(base), sh.gen if self.wrong == "presence" else 0)
        if key not in self.cache: self.cache[key] = (base, self._wrongly(base, state))
        return self.cache[key][1]

    def _wrongly(self, base, state):
        sh, rec = self.sh, dict(base)
        if self.wrong == "dead": rec["alive"] = np.ones(base["len"], dtype=bool)
        if self.wrong == "res" and state != LIVE: rec["res"] = sh.prev_res[state]
        if self.wrong == "presence":
            live = self._live()
            rec["present"] = {c: _fit(live["present"][c], base["len"]) for c in base["present"]}
        if self.wrong == "len":
            longer = [r for r in sh.recs.values() if r["len"] > base["len"]]
            if longer:
                d = max(longer, key=lambda r: r["len"]); n, m = base["len"], d["len"]
                rec["len"] = m
                rec["alive"] = np.concatenate([base["alive"][:n], d["alive"][n:m]])
                rec["present"] = {c: np.concatenate([base["present"][c][:n], d["present"][c][n:m]]) for c in base["present"]}
                rec["words"] = rec["columns"] = {k: np.concatenate([base["words"][k][:n], d["words"][k][n:m]]) for k in base["words"]}
        return rec

    def _m(self, key, recs, fn):
        k = key + tuple(id(r) for r in recs)
        if k not in self.sh.memo: self.sh.memo[k] = (recs, fn())
        return self.sh.memo[k][1]

    def snapshot_copy(self, f): return Block(self._rec(f))

    def checksum_parts(self, state):
        rec = self._rec(state)
        m = self._m(("parts",), (rec,), lambda: cp.model_parts(rec, self.sh.cfg.specs))
        return ChecksumParts(parts=dict(m["parts"]), counts=dict(m["counts"]), len=m["len"], active=m["active"], checksum=m["checksum"])

    def diff(self, a, b, *, max_entries=64, trust_versions=False):
        ra, rb = self._rec(a), self._rec(b)
        m = self._m(("diff", max_entries), (ra, rb), lambda: sd.model_diff(ra, rb, self.sh.cfg.comps, max_entries))
        bits = lambda x: [i for i in range(64) if (x >> i) & 1]
        none = lambda x: None if x == sd.NO_WORD else x
        es = [DiffEntry(slot=s, alive_a=bool(aa), alive_b=bool(ab), presence_diff=bits(pd), column_diff=bits(cd), first_comp=none(fc), first_word=none(fw), first_a=fa, first_b=fb)
              for s, aa, ab, pd, cd, fc, fw, fa, fb in m["entries"]]
        return StateDiff(len_a=m["len_a"], len_b=m["len_b"], n_entities=m["n_entities"], n_alive=m["n_alive"], n_presence=dict(m["n_presence"]), n_value=dict(m["n_value"]),
                         resource_diff=list(m["resource_diff"]), entries=es)

    def query_bytes(self, state, desc, max_rows, extra=512):
        rec = self._rec(state)
        wbs = qc.word_bytes_of(self.sh, desc)
        m = qc.model_of(rec, desc, max_rows)
        return m["n_matched"], m["n_rows"], qc.expected_buffer(m, wbs, max_rows, qc.model_layout(wbs, desc["slots"], max_rows)[2] + extra)

    def query(self, state, fetch, *, with_=(), without=(), slots=True, max_rows=None, out=None):
        named = {c for c, _ in fetch} | set(with_) | set(without)
        if state != LIVE and named & self.sh.cfg.no_rollback:
            raise bg.GgrsHipError(-1, f"a query of a snapshot names component {min(named & self.sh.cfg.no_rollback)}, which is not registered for rollback")
        raise NotImplementedError("the shadow serves whole buffers: query_bytes")


class Teeth:
    """One witness per view of one ShadowInspector, all shown the same session: the true view's witness must pass (its failure is the test's), a wrong view's
    witness that fails is noted in `failed` and shown nothing more."""

    def __init__(self):
        self.cfg = iw.Witness()
        self.inner = {name: iw.Witness() for name in (None,) + WRONG}
        self.memo, self.failed, self.views = {}, {}, None
        for w in self.inner.values(): w.memo = self.memo

    def scenario(self, sc):
        for w in (self.cfg, *self.inner.values()): w.scenario(sc)

    def watch(self, world):
        for w in (self.cfg, *self.inner.values()): world = w.watch(world)
        return world

    cks = property(lambda self: self.cfg.cks)

    @cks.setter
    def cks(self, v):
        for w in (self.cfg, *self.inner.values()): w.cks = v

    def shadow(self, world):
        sh = ShadowInspector(world, self.cfg)
        self.views = {name: sh.view(name) for name in self.inner}
        return sh

    def _each(self, method, A, *args, **kw):
        shared = {}
        for name, w in self.inner.items():
            if name in self.failed: continue
            w._shared = shared
            try: getattr(w, method)(A, self.views[name], *args, **kw)
            except AssertionError as e:
                if name is None: raise
                self.failed[name] = str(e).split("\n")[0][:160]

    def on_list(self, A, B, reqs, checksums, in_flight=False): self._each("on_list", A, reqs, checksums, in_flight=in_flight)
    def before_sweep(self, A, B, frames): self._each("before_sweep", A, frames)
    def on_sweep_frame(self, A, B, f): self._each("on_sweep_frame", A, f)
    def after_sweep(self, A, B, ctx): self._each("after_sweep", A, ctx); self.memo.clear()

    hit = property(lambda self: self.inner[None].hit)


def make_shadow(family, teeth):
    """backend B of one case: the REFSHAPED oracle (adapter) under a ShadowInspector, behind enqueue / collect."""
    if iw.FAMILIES[family] is not None: return lambda sc: InFlight(teeth.shadow(OracleWorld(sc.capacity, 8, REFSHAPED)))
    if family.startswith("colony"): return lambda sc: fd.InFlight(teeth.shadow(sc.oracle(REFSHAPED)))
    return lambda sc: fu.InFlight(teeth.shadow(sc.oracle(REFSHAPED)))


_SESSIONS = {}


def session(family, seed):
    """One committed case, run once and shared: {"log", "hit": the classes as pinned in inspect_witness.HIT, "failed": wrong inspector -> its witness's first complaint}."""
    key = (family, seed)
    if key not in _SESSIONS:
        t = Teeth()
        log = iw.run_case(family, seed, make_shadow(family, t), t)
        w = t.inner[None]
        assert w.sweeps == 2 and w.sync_lists >= 1 and w.asked > 20, (log[0], w.sweeps, w.sync_lists, w.asked)
        _SESSIONS[key] = {"log": log, "hit": iw.letters(t.hit), "failed": dict(t.failed), "twice": fu.shapes(log)[1]}
    return _SESSIONS[key]


ALL_CASES = [(f, s) for f, seeds in iw.CASES.items() for s in seeds]


@pytest.mark.parametrize("family,seed", ALL_CASES, ids=[f"{f}-{s}" for f, s in ALL_CASES])
def test_the_witness_passes_on_the_shadow_inspector_and_hits_what_is_pinned(family, seed):
    s = session(family, seed)
    assert s["hit"] == iw.HIT[family, seed], (s["log"][0], s["hit"])


def _by_group():
    out = {}
    for f, s in ALL_CASES: out.setdefault(group(f), []).append(session(f, s))
    return out


def test_every_wrong_inspector_is_caught_in_every_family_that_can_show_it():
    by = _by_group()
    assert set(by) == set(_ALL)
    for wrong in WRONG:
        for g in TEETH[wrong]:
            caught = sum(wrong in s["failed"] for s in by[g])
            print(f"{wrong} in {g}: caught in {caught}/{len(by[g])} sessions")
            assert caught >= 3, (wrong, g, caught)
    for g, ss in by.items():                                 # "saved twice" wherever the logs advance a frame twice
        assert sum(s["twice"] > 0 for s in ss) >= 3, g


def test_coverage_floors_of_the_committed_seeds():
    by = _by_group()
    for g, classes in FLOORS.items():
        for c in classes:
            n = sum(iw.CLASSES.index(c) in [iw.LETTERS.index(x) for x in s["hit"]] for s in by[g])
            print(f"{g}: {c} in {n}/{len(by[g])} sessions")
            assert n >= 3, (g, c, n)


def test_the_forced_deferral_seeds_defer_and_are_read():
    """What the GPU tier asserts of every `plain` session -- Saves were deferred, an owed slot was materialised -- must follow from the stream alone:
    fuzz_util.deferral_model counts two groups at least that MUST defer and a Load of an owed frame (the witness's calls come before it and find the debt)."""
    for seed in iw.CASES["plain"]:
        s = session("plain", seed)
        depth = int(s["log"][0].split("depth=")[1].split()[0])
        groups, reads = fuzz_util.deferral_model(s["log"], depth)
        assert groups >= 2 and reads >= 1, (seed, groups, reads)


def test_the_case_table_holds_the_session_counts_per_family():
    n = {g: sum(len(iw.CASES[f]) for f in iw.CASES if group(f) == g) for g in _ALL}
    assert n["box"] == 6 and n["plain"] == 8 and n["tagged"] == 8 and n["spawn"] == 4 and n["brand"] == 8 + 1 and n["colony"] == 8 + 1 and n["skirmish"] == 10 + 1, n
    assert set(iw.HIT) == set(ALL_CASES)
