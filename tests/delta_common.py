"""The delta tests' shared pieces (ggrs_hip_delta_frames / ggrs_hip_delta_block; include/ggrs_hip.h "DELTA").

    model_delta      the semantics restated in numpy over two records in the form query_common.record produces -- len, alive, presence, words per side -- with
                     no knowledge of blocks, tiles or kernels.  The layout of the output buffer is the query's: query_common.expected_buffer / model_layout
    wrong_model      the same with one deliberate mistake (WRONG names them): what the committed cases must tell from the model
    device_delta     World.delta into a buffer pre-filled with FILL, as (report fields, bytes)
(A helper module, no tests of its own.)"""
import numpy as np

import query_common as qc

KINDS = ("changed", "added", "removed", "despawned")
NEW_BASED = ("changed", "added")
WRONG = ("ignores_old_alive", "compares_slots_dead_on_both_sides", "absent_on_both_sides_is_changed")


def make_delta(kind, changed=(), fetch=(), with_=(), without=(), slots=True):
    """changed: component ids; fetch: (comp, word) pairs.  The filter and the fetch are a query desc, judged on the base side."""
    assert kind in KINDS
    return {"kind": kind, "changed": set(changed), "q": qc.make_desc(fetch, with_, without, slots)}


def _cut(mask, len_, n):
    """A side's mask as bool[n]: bits at or beyond the side's len are clear (a slot there is dead on that side)."""
    return qc.as_bits(qc.as_bits(mask, len_), n)


def _words(col, n):
    col = np.asarray(col)
    assert col.dtype.kind == "u", "words are bits: hand them over as unsigned integers"
    return col[:n] if col.size >= n else np.concatenate([col, np.zeros(n - col.size, dtype=col.dtype)])


def _model(rec_new, rec_old, desc, max_rows, bug=None):
    kind, q = desc["kind"], desc["q"]
    base, other = (rec_new, rec_old) if kind in NEW_BASED else (rec_old, rec_new)
    n = base["len"]                                                                # rows come from the base side: slots below its len
    a_base, a_other = _cut(base["alive"], base["len"], n), _cut(other["alive"], other["len"], n)
    if bug == "ignores_old_alive":                                                 # every slot below old's len counts as alive there
        a_old = _cut(np.ones(rec_old["len"], dtype=bool), rec_old["len"], n)
        a_base, a_other = (a_base, a_old) if kind in NEW_BASED else (a_old, a_other)
    filt = np.ones(n, dtype=bool) if bug == "compares_slots_dead_on_both_sides" else a_base.copy()
    for c in sorted(q["with"] | {c for c, _ in q["fetch"]}): filt &= qc.as_bits(base["present"][c], n)
    for c in sorted(q["without"]): filt &= ~qc.as_bits(base["present"][c], n)
    if kind == "despawned":
        assert not desc["changed"], "DESPAWNED asks about no component"
        match = filt & ~a_other
    else:
        assert desc["changed"], "CHANGED, ADDED and REMOVED ask about at least one component"
        match = np.zeros(n, dtype=bool)
        for c in sorted(desc["changed"]):
            raw_b, raw_o = qc.as_bits(base["present"][c], n), qc.as_bits(other["present"][c], n)
            p_base, p_other = (raw_b if bug == "compares_slots_dead_on_both_sides" else a_base & raw_b), a_other & raw_o
            hit = p_base & ~p_other                                                # added (new-based) or removed (old-based): present here, not there
            if kind == "changed":
                common = p_base & p_other
                if bug == "absent_on_both_sides_is_changed": common = common | (~raw_b & ~raw_o)
                for key in sorted(k for k in base["columns"] if k[0] == c):
                    hit |= common & (_words(base["columns"][key], n) != _words(other["columns"][key], n))      # bits: -0.0 != 0.0, NaN payloads count
            match |= hit
        match &= filt
    slots = np.flatnonzero(match)
    n_rows = min(int(slots.size), int(max_rows))
    rows = slots[:n_rows]
    return {"n_matched": int(slots.size), "n_rows": n_rows, "slots": rows.astype(qc.U32) if q["slots"] else None,
            "columns": [_words(base["columns"][key], n)[rows].copy() for key in q["fetch"]], "all_slots": slots,
            "len_new": rec_new["len"], "len_old": rec_old["len"], "n_beyond_old_len": int((slots >= rec_old["len"]).sum()) if kind in NEW_BASED else 0}


def model_delta(rec_new, rec_old, desc, max_rows):
    """The rows ggrs_hip_delta_* gathers for `desc` (make_delta) between two records, and its report: n_matched exact, the first min(n_matched, max_rows) rows
    ("all_slots": every matched slot, whatever max_rows is)."""
    return _model(rec_new, rec_old, desc, max_rows)


def wrong_model(bug):
    assert bug in WRONG
    return lambda rec_new, rec_old, desc, max_rows: _model(rec_new, rec_old, desc, max_rows, bug=bug)


def same_answer(a, b):
    """Two model results say the same: counts, rows, words."""
    if (a["n_matched"], a["n_rows"], a["n_beyond_old_len"]) != (b["n_matched"], b["n_rows"], b["n_beyond_old_len"]): return False
    if (a["slots"] is None) != (b["slots"] is None) or (a["slots"] is not None and not np.array_equal(a["slots"], b["slots"])): return False
    return all(np.array_equal(x, y) for x, y in zip(a["columns"], b["columns"]))


# ---------------------------------------------------------------------------------------------------------------- the device
def word_bytes_of(w, desc): return [w._comps[c][1] for c, _ in desc["q"]["fetch"]]


def device_delta(w, new, old, desc, max_rows, extra=512, trust_versions=False):
    """World.delta into a buffer pre-filled with FILL (`extra` bytes longer than the layout asks for): ((n_matched, n_rows, n_beyond_old_len, len_new, len_old), bytes)."""
    import torch
    q = desc["q"]
    _, _, total = qc.model_layout(word_bytes_of(w, desc), q["slots"], max_rows)
    out = torch.full((total + extra,), qc.FILL, dtype=torch.uint8, device=f"cuda:{w.device}")
    r = w.delta(new, old, q["fetch"], kind=desc["kind"], changed=desc["changed"], with_=q["with"], without=q["without"], slots=q["slots"], max_rows=max_rows, out=out,
                trust_versions=trust_versions)
    assert r.buffer is out and r.n_rows == min(r.n_matched, max_rows)
    return (r.n_matched, r.n_rows, r.n_beyond_old_len, r.len_new, r.len_old), out.cpu().numpy()


def assert_answer_equals_model(w, got, want, desc, max_rows, ctx=""):
    """What device_delta returned against a model result, bit for bit (rows, the bytes beyond them and the padding)."""
    rep, buf = got
    exp_rep = (want["n_matched"], want["n_rows"], want["n_beyond_old_len"], want["len_new"], want["len_old"])
    assert rep == exp_rep, (ctx, desc["kind"], rep, exp_rep)
    exp = qc.expected_buffer(want, word_bytes_of(w, desc), max_rows, buf.size)
    if not np.array_equal(buf, exp):
        bad = np.flatnonzero(buf != exp)
        raise AssertionError(f"{ctx} {desc['kind']}: output buffer differs from the model at {bad.size} bytes, first at {bad[:8]}: {buf[bad[:8]]} vs {exp[bad[:8]]}")


def assert_delta_equals_model(w, new, old, rec_new, rec_old, desc, max_rows, ctx="", **kw):
    want = model_delta(rec_new, rec_old, desc, max_rows)
    assert_answer_equals_model(w, device_delta(w, new, old, desc, max_rows, **kw), want, desc, max_rows, ctx)
    return want
