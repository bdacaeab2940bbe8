"""The scatter tests' shared pieces (ggrs_hip_scatter; World.scatter; include/ggrs_hip.h "SCATTER").

    make_sdesc       a scatter as the tests name it: op, the (comp, word) pairs its rows carry, the components a remove removes
    model_scatter    the semantics restated in numpy over a query_common.record-style snapshot of a world's downloads -- alive, presence, words -- with no
                     knowledge of blocks, tiles or kernels: (the record after the call, the report)
    apply_per_slot   the same edit through the calls a host has today -- despawn, insert_component, remove_component one slot at a time, download_word +
                     upload_word per written word -- and only for the rows the model applies: what the oracle world gets in every comparison
    full_record      a world's live state over [0, capacity): every word of every component, the alive mask and every presence mask, so that untouched slots
                     and columns are part of every comparison
    world_scatter    World.scatter with the model's arguments, as the model's report (a refusal of the rows included)
(A helper module, no tests of its own.)"""
import numpy as np

import bevy_ggrs_amd as bg
import query_common as qc

OPS = ("write", "insert", "remove", "despawn")
UINT = qc.UINT


def make_sdesc(op, words=(), comps=()):
    assert op in OPS
    return {"op": op, "words": [tuple(int(x) for x in w) for w in words], "comps": set(int(c) for c in comps)}


# ---------------------------------------------------------------------------------------------------------------- the model
def _bits(mask):
    """A mask as a bool array of all its bits: from bools, or from the uint64 words the download calls fill."""
    m = np.asarray(mask)
    if m.dtype == np.uint64: return np.unpackbits(m.view(np.uint8), bitorder="little").astype(bool)
    return m.astype(bool).copy()


def copy_record(rec):
    """A deep copy with every mask as bools."""
    return {"len": int(rec["len"]), "alive": _bits(rec["alive"]), "present": {c: _bits(m) for c, m in rec["present"].items()},
            "columns": {k: np.array(v, copy=True) for k, v in rec["columns"].items()}}


def first_bad_row(len_, slots):
    """The lowest row whose slot is at or beyond len or whose predecessor's slot is not smaller; None when the rows are strictly ascending slots below len."""
    s = np.asarray(slots).astype(np.int64).reshape(-1)
    bad = s >= len_
    bad[1:] |= s[:-1] >= s[1:]
    hit = np.flatnonzero(bad)
    return int(hit[0]) if hit.size else None


def verdicts(rec, desc, slots):
    """(applied, dead, absent) as bool arrays over the rows -- judged on `rec`, the state before the call; the rows must be valid."""
    s = np.asarray(slots).astype(np.int64).reshape(-1)
    alive = _bits(rec["alive"])[s] if s.size else np.zeros(0, dtype=bool)
    have = np.ones(s.size, dtype=bool)
    if desc["op"] == "write":
        for c in sorted({c for c, _ in desc["words"]}): have &= _bits(rec["present"][c])[s]
    return alive & have, ~alive, alive & ~have


def model_scatter(record, desc, slots, columns=()):
    """record: {"len", "alive", "present": {c: mask}, "columns": {(c, w): unsigned array}} (masks as bools or uint64 words, arrays at least len long).
    desc: make_sdesc(..).  slots: the rows' slots; columns[k]: the rows' values of desc["words"][k] (write, insert).
    Returns (the record after the call, {"len", "n_rows", "n_applied", "n_dead", "n_absent", "first_bad_row"}).  Rows that are not strictly ascending slots below
    len: first_bad_row is the lowest offender, every count is 0 and the record is unchanged."""
    out = copy_record(record)
    s = np.asarray(slots).astype(np.int64).reshape(-1)
    rep = {"len": out["len"], "n_rows": int(s.size), "n_applied": 0, "n_dead": 0, "n_absent": 0, "first_bad_row": first_bad_row(out["len"], s)}
    if rep["first_bad_row"] is not None: return out, rep
    applied, dead, absent = verdicts(record, desc, s)
    rep.update(n_applied=int(applied.sum()), n_dead=int(dead.sum()), n_absent=int(absent.sum()))
    on = s[applied]
    op = desc["op"]
    if op in ("write", "insert"):
        assert len(columns) == len(desc["words"])
        for key, col in zip(desc["words"], columns):
            col = np.asarray(col).reshape(-1)
            assert col.dtype.kind == "u" and col.dtype == out["columns"][key].dtype and col.size == s.size, "words are bits: unsigned integers of the word's width, one per row"
            out["columns"][key][on] = col[applied]
    if op == "insert":
        for c in {c for c, _ in desc["words"]}: out["present"][c][on] = True
    elif op == "remove":
        for c in desc["comps"]: out["present"][c][on] = False
    elif op == "despawn":
        out["alive"][on] = False
    return out, rep


def assert_records_equal(a, b, ctx=""):
    """Two records bit for bit: len, the alive mask, every presence mask, every word of every column (masks of different lengths: the longer one's tail is 0)."""
    assert int(a["len"]) == int(b["len"]), (ctx, "len", a["len"], b["len"])

    def same_mask(x, y, what):
        x, y = _bits(x), _bits(y)
        n = max(x.size, y.size)
        x, y = np.pad(x, (0, n - x.size)), np.pad(y, (0, n - y.size))
        if not np.array_equal(x, y):
            bad = np.flatnonzero(x != y)
            raise AssertionError(f"{ctx}: {what} differs at {bad.size} slots, first {bad[:8]}")
    same_mask(a["alive"], b["alive"], "alive")
    assert a["present"].keys() == b["present"].keys() and a["columns"].keys() == b["columns"].keys(), ctx
    for c in a["present"]: same_mask(a["present"][c], b["present"][c], f"presence of component {c}")
    for k in a["columns"]:
        x, y = np.asarray(a["columns"][k]), np.asarray(b["columns"][k])
        assert x.dtype == y.dtype and x.size == y.size, (ctx, k, x.dtype, y.dtype, x.size, y.size)
        if not np.array_equal(x, y):
            bad = np.flatnonzero(x != y)
            raise AssertionError(f"{ctx}: word {k} differs at {bad.size} slots, first {bad[:8]}: {x[bad[:4]]} vs {y[bad[:4]]}")


# ---------------------------------------------------------------------------------------------------------------- the worlds
def full_record(w):
    """The live state over [0, capacity) through the download calls: every word, the alive mask, every presence mask."""
    cap = int(w.capacity)
    rec = {"len": w.len, "alive": w.alive_mask(cap), "present": {}, "columns": {}}
    for c, (_, _, nw) in enumerate(w._comps):
        rec["present"][c] = w.present_mask(c, cap)
        for k in range(nw): rec["columns"][(c, k)] = w.download_word(c, k, 0, cap)
    return rec


def mask_record(w, comps):
    """What the verdicts need: len, the alive mask and the presence masks of `comps` over [0, len)."""
    n = w.len
    return {"len": n, "alive": w.alive_mask(n), "present": {c: w.present_mask(c, n) for c in comps}, "columns": {}}


def apply_per_slot(world, desc, slots, columns=()):
    """The edit of model_scatter through the calls a host has without the bulk call, only for the rows the model applies (judged on the world as it is now):
    write: download_word, merge, upload_word per word; insert / remove / despawn: one single-slot call per applied row and component.  Rows the model refuses
    leave the world alone.  Returns the model's report."""
    s = np.asarray(slots).astype(np.int64).reshape(-1)
    op = desc["op"]
    named = sorted({c for c, _ in desc["words"]} | desc["comps"])
    rec = mask_record(world, named)
    rep = {"len": rec["len"], "n_rows": int(s.size), "n_applied": 0, "n_dead": 0, "n_absent": 0, "first_bad_row": first_bad_row(rec["len"], s)}
    if rep["first_bad_row"] is not None or s.size == 0: return rep
    applied, dead, absent = verdicts(rec, desc, s)
    rep.update(n_applied=int(applied.sum()), n_dead=int(dead.sum()), n_absent=int(absent.sum()))
    on = s[applied]
    if on.size == 0: return rep
    cols = [np.asarray(c).reshape(-1)[applied] for c in columns]
    if op == "write":
        lo, hi = int(on.min()), int(on.max()) + 1
        for key, col in zip(desc["words"], cols):
            cur = world.download_word(key[0], key[1], lo, hi - lo)
            cur[on - lo] = col
            world.upload_word(key[0], key[1], lo, cur)
    elif op == "insert":
        for c in sorted({c for c, _ in desc["words"]}):
            _, wb, nw = world._comps[c]
            by_word = {k: cols[i] for i, (cc, k) in enumerate(desc["words"]) if cc == c}
            assert sorted(by_word) == list(range(nw)), "an insert names every word of the component"
            for r, slot in enumerate(on): world.insert_component(c, int(slot), np.array([by_word[k][r] for k in range(nw)], dtype=UINT[wb]))
    elif op == "remove":
        for c in sorted(desc["comps"]):
            for slot in on: world.remove_component(c, int(slot))
    else:
        for slot in on: world.despawn(int(slot))
    return rep


def world_scatter(w, desc, slots, columns=()):
    """World.scatter of the model's arguments, as the model's report: a refusal of the rows comes back as first_bad_row (the package raises GgrsHipError
    with the report attached), everything else raises."""
    values = {key: np.asarray(col) for key, col in zip(desc["words"], columns)}
    try:
        r = w.scatter(np.asarray(slots, dtype=np.uint32), values if desc["op"] in ("write", "insert") else None, op=desc["op"], comps=sorted(desc["comps"]))
    except bg.GgrsHipError as e:
        rep = getattr(e, "report", None)
        if rep is None or rep.first_bad_row is None: raise
        assert e.code == bg.GGRS_E_INVALID and f"first_bad_row {rep.first_bad_row}" in str(e), str(e)
        r = rep
    return {"len": r.len, "n_rows": r.n_rows, "n_applied": r.n_applied, "n_dead": r.n_dead, "n_absent": r.n_absent, "first_bad_row": r.first_bad_row}
