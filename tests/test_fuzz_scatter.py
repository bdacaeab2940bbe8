"""CPU tier of the scatter fuzz (tests/fuzz_scatter.py), so that the GPU tier (test_gpu_zfuzz_scatter.py) cannot go hollow.  Every committed case runs once
here with the FLAT oracle (adapter) as backend A -- edited one slot at a time -- and, as backend B behind enqueue / collect (the stream the HIP backend gets), a
second oracle world behind a ModelShim whose `scatter` is scatter_common.model_scatter over the world's downloads.

  * plumbing: the fuzzer's comparisons and the scenarios' own (reports, the raw bits of rows that were not applied) pass in every session;
  * coverage floors, counted from the oracle's verdicts and the log alone: in every family each of the four ops, a dead row, an absent row, rows of one unit in
    two waves, a refused call, an edit behind a list in flight and an edit a later Load takes back occur at least once, and EVERY seed holds two bulk edits at least;
  * teeth: four deliberately wrong shims -- one that writes dead slots, one that forgets the presence bit on INSERT, one that ignores absence on WRITE, one that
    applies the rows behind a bad row -- are each caught in every family."""
import numpy as np
import pytest

import bevy_ggrs_amd as bg
import fuzz_scatter as fs
import fuzz_user_worlds as fu
import scatter_common as sc
from oracle.binding import REFSHAPED, OracleWorld
from test_fuzz_requests import InFlight

WRONG = ("dead", "no_presence", "ignore_absent", "after_bad")
FLOORS = ("write", "insert", "remove", "despawn", "dead", "absent", "two_waves", "bad", "in_flight", "rolled_back")


class ModelShim:
    """A backend (an oracle world behind enqueue / collect) with World.scatter served by the numpy model: the named columns and masks are downloaded, the model
    runs, what it changed is written back through the single-slot calls.  `wrong` names the one thing it gets deliberately wrong."""

    def __init__(self, world, wrong=None): self.__dict__.update(_w=world, wrong=wrong)

    def __getattr__(self, k): return getattr(self._w, k)

    def pending_batches(self): return len(self._w._q)

    def scatter(self, rows, values=None, *, op="write", comps=()):
        w, wrong = self._w, self.wrong
        values = dict(values or {})
        desc = sc.make_sdesc(op, list(values), comps)
        slots = np.asarray(rows).astype(np.int64).reshape(-1)
        cols = [np.asarray(v) for v in values.values()]
        n = w.len
        named = sorted({c for c, _ in desc["words"]} | desc["comps"])
        rec = {"len": n, "alive": w.alive_mask(n), "present": {c: w.present_mask(c, n) for c in named}, "columns": {key: w.download_word(key[0], key[1], 0, n) for key in desc["words"]}}
        seen = sc.copy_record(rec)
        if wrong == "dead": seen["alive"][:] = True
        if wrong == "ignore_absent" and op == "write":
            for c in seen["present"]: seen["present"][c][:] = True
        bad = sc.first_bad_row(n, slots)
        use, use_cols = slots, cols
        if bad is not None and wrong == "after_bad":                             # the rows that are fine by themselves go in all the same
            keep, top = [], -1
            for i, s in enumerate(slots):
                if top < s < n: keep.append(i); top = int(s)
            use, use_cols = slots[keep], [c[keep] for c in cols]
        out, rep = sc.model_scatter(seen, desc, use, use_cols)
        if wrong == "dead": out["alive"] &= sc._bits(rec["alive"])               # (it writes dead slots; it does not resurrect them)
        if (wrong == "ignore_absent" and op == "write") or (wrong == "no_presence" and op == "insert"): out["present"] = {c: sc._bits(m) for c, m in rec["present"].items()}
        self._write_back(rec, out)
        if bad is not None:
            e = bg.GgrsHipError(bg.GGRS_E_INVALID, f"scatter rows must be strictly ascending slots below len {n}: first_bad_row {bad}")
            e.report = bg.ScatterReport(len=n, n_rows=int(slots.size), n_applied=0, n_dead=0, n_absent=0, first_bad_row=bad)
            raise e
        return bg.ScatterReport(len=n, n_rows=rep["n_rows"], n_applied=rep["n_applied"], n_dead=rep["n_dead"], n_absent=rep["n_absent"], first_bad_row=None)

    def _write_back(self, before, after):
        w, n = self._w, before["len"]
        for c in after["present"]:
            was, now = sc._bits(before["present"][c])[:n], after["present"][c][:n]
            nw = w._comps[c][2]
            for s in np.flatnonzero(now & ~was):
                words = [after["columns"][(c, k)][s] if (c, k) in after["columns"] else w.download_word(c, k, int(s), 1)[0] for k in range(nw)]
                w.insert_component(c, int(s), np.array(words, dtype=sc.UINT[w._comps[c][1]]))
            for s in np.flatnonzero(was & ~now): w.remove_component(c, int(s))
        for key, col in after["columns"].items():
            ch = np.flatnonzero(col[:n] != before["columns"][key][:n])
            if ch.size: w.upload_word(key[0], key[1], int(ch[0]), col[int(ch[0]):int(ch[-1]) + 1])
        for s in np.flatnonzero(sc._bits(before["alive"])[:n] & ~after["alive"][:n]): w.despawn(int(s))


def make_shim(family, wrong=None):
    if fs.group(family) == "skirmish": return lambda sc_: ModelShim(fu.InFlight(sc_.oracle(REFSHAPED)), wrong)
    return lambda sc_: ModelShim(InFlight(OracleWorld(sc_.capacity, 8, REFSHAPED)), wrong)


_SESSIONS = {}


def session(family, seed):
    key = (family, seed)
    if key not in _SESSIONS:
        log, scn = fs.run_case(family, seed, make_shim(family))
        cov = dict(scn.cov); cov["rolled_back"] = fs.rolled_back(log)
        _SESSIONS[key] = {"log": log, "cov": cov, "n_bulk": scn.n_bulk, "n": scn.n}
    return _SESSIONS[key]


@pytest.mark.parametrize("mode,family,seed", fs.ALL_CASES, ids=[f"{m}-{f}-{s}" for m, f, s in fs.ALL_CASES])
def test_the_model_shim_holds_against_the_oracle_edited_per_slot(mode, family, seed):
    s = session(family, seed)
    print(s["log"][0], s["n_bulk"], s["cov"])
    assert s["n_bulk"] >= 2, (s["log"][0], s["n_bulk"])                           # the per-seed floor
    assert s["n_bulk"] == sum(line.startswith("scatter ") for line in s["log"][1:])
    if family.endswith("_tile"): assert s["n"] >= fs.TILE_MIN, s["log"][0]


def test_coverage_floors_of_every_family():
    by = {}
    for _, f, s in fs.ALL_CASES: by.setdefault(fs.group(f), []).append(session(f, s))
    assert set(by) == {"particles", "generic", "skirmish"}
    for g, ss in by.items():
        for c in FLOORS:
            n = sum(bool(s["cov"].get(c)) for s in ss)
            print(f"{g}: {c} in {n}/{len(ss)} sessions")
            assert n >= 1, (g, c)


def test_the_case_table_holds_the_session_counts():
    n = {m: len(c) for m, c in fs.CASES.items()}
    assert n == {"default": 16, "tags_lazy": 8, "deferral": 8, "tile": 4} and len(set(fs.ALL_CASES)) == 36


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_shim_is_caught_in_every_family(wrong):
    for g in ("particles", "generic", "skirmish"):
        caught = None
        for _, f, seed in fs.ALL_CASES:
            if fs.group(f) != g or f.endswith("_tile"): continue
            try: fs.run_case(f, seed, make_shim(f, wrong))
            except AssertionError as e:
                caught = (f, seed, str(e).split("\n")[0][:200]); break
        print(f"{wrong} in {g}: {caught}")
        assert caught, (wrong, g)
