"""The sorted-query tests' shared pieces (ggrs_hip_query_sorted / ggrs_hip_query_sorted_block; include/ggrs_hip.h "SORTED QUERY").

    key_image            a key word's order-preserving unsigned image at its width: U the bits, I the bits ^ the sign bit, F the bits ^ (sign set ? all ones : the
                         sign bit), "desc" the complement of that -- restated from the header, in numpy over uint64
    model_query_sorted   the semantics: query_common.model_query selects the rows (a key's component counts as With), np.lexsort over the images and the slot
                         orders them, max_rows keeps the first rows of the full order
    device_query_sorted  World.query_sorted into a buffer pre-filled with FILL, as (n_matched, n_rows, bytes)
    plant_widths         the widths world of query_common.build_widths with values planted for sorting: NaNs of both signs with different payloads, +-0, +-inf,
                         denormals, integers across the sign, one column with 5 distinct values
(A helper module, no tests of its own.)"""
import numpy as np

import query_common as qc
from query_common import U8, U16, U32, U64, UINT, expected_buffer  # noqa: F401  (expected_buffer is reused as it is)

MASK = {1: 0xFF, 2: 0xFFFF, 4: 0xFFFFFFFF, 8: 0xFFFFFFFFFFFFFFFF}


def key_image(col, wb, kind, desc=False):
    v = np.asarray(col).astype(U64)
    mask, sign = U64(MASK[wb]), U64(1 << (8 * wb - 1))
    if kind == "u": t = v
    elif kind == "i": t = v ^ sign
    elif kind == "f":
        assert wb in (4, 8), "F keys are 4- and 8-byte words"
        t = np.where((v & sign) != 0, v ^ mask, v ^ sign)
    else: raise ValueError(kind)
    return (~t & mask) if desc else t


def norm_key(key):
    """(comp, word, kind, descending) of an order_by item."""
    assert len(key) in (3, 4) and (len(key) == 3 or key[3] == "desc"), key
    return int(key[0]), int(key[1]), key[2], len(key) == 4


def model_query_sorted(rec, desc, order_by, max_rows, word_bytes=None):
    """rec: query_common.record's dict; desc: query_common.make_desc; order_by: (comp, word, kind[, "desc"]) items, the most significant first.  word_bytes[(c, w)]
    defaults to the column's dtype.  Returns model_query's dict, rows in sorted order."""
    keys = [norm_key(k) for k in order_by]
    assert 1 <= len(keys) <= 4
    sel = qc.make_desc(desc["fetch"], desc["with"] | {c for c, _, _, _ in keys}, desc["without"], slots=True)
    everyone = qc.model_query(rec["alive"], rec["len"], rec["present"], rec["columns"], sel, rec["len"])
    slots = everyone["slots"].astype(np.int64)
    images = []
    for c, w, kind, dsc in keys:
        col = np.asarray(rec["columns"][(c, w)])
        wb = col.dtype.itemsize if word_bytes is None else word_bytes[(c, w)]
        images.append(key_image(col[slots], wb, kind, dsc))
    order = np.lexsort([slots] + images[::-1])                                  # (lexsort: the LAST key is the primary one)
    n_rows = min(int(slots.size), int(max_rows))
    rows = slots[order][:n_rows]
    cols = [np.asarray(rec["columns"][key])[rows].copy() for key in desc["fetch"]]
    return {"n_matched": int(slots.size), "n_rows": n_rows, "slots": rows.astype(U32) if desc["slots"] else None, "columns": cols}


# ---------------------------------------------------------------------------------------------------------------- the device
def device_query_sorted(w, state, desc, order_by, max_rows, extra=512):
    import torch
    _, _, total = qc.model_layout(qc.word_bytes_of(w, desc), desc["slots"], max_rows)
    out = torch.full((total + extra,), qc.FILL, dtype=torch.uint8, device=f"cuda:{w.device}")
    r = w.query_sorted(state, desc["fetch"], order_by, with_=desc["with"], without=desc["without"], slots=desc["slots"], max_rows=max_rows, out=out)
    assert r.buffer is out and r.n_rows == min(r.n_matched, max_rows)
    return r.n_matched, r.n_rows, out.cpu().numpy()


def assert_sorted_equals_model(w, state, rec, desc, order_by, max_rows, ctx=""):
    """The device's whole buffer against the model's, bit for bit (rows, the bytes beyond them and the padding); returns (the model's result, the buffer)."""
    want = model_query_sorted(rec, desc, order_by, max_rows)
    n_matched, n_rows, buf = device_query_sorted(w, state, desc, order_by, max_rows)
    assert (n_matched, n_rows) == (want["n_matched"], want["n_rows"]), (ctx, n_matched, n_rows, want["n_matched"], want["n_rows"])
    exp = expected_buffer(want, qc.word_bytes_of(w, desc), max_rows, buf.size)
    if not np.array_equal(buf, exp):
        bad = np.flatnonzero(buf != exp)
        raise AssertionError(f"{ctx}: output buffer differs from the model at {bad.size} bytes, first at {bad[:8]}: {buf[bad[:8]]} vs {exp[bad[:8]]}")
    return want, buf


# ---------------------------------------------------------------------------------------------------------------- planted values
F32_SPECIALS = np.array([0x7FC00000, 0x7FC00001, 0x7F800001, 0xFFC00000, 0xFFC00123, 0xFF800001,           # NaNs of both signs, different payloads
                         0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,   # +-0, +-inf, denormals
                         0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF], dtype=U32)
F64_SPECIALS = np.array([0x7FF8000000000000, 0x7FF8000000000001, 0x7FF0000000000001, 0xFFF8000000000000, 0xFFF8000000000123, 0xFFF0000100000000,
                         0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001, 0x8000000000000001,
                         0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF, 0x3FF0000000000000, 0xBFF0000000000000, 0x3FF0000000000001, 0x3FF0000100000000], dtype=U64)


def planted_columns(n, first=0):
    """The widths world's words for slots first .. first + n: {component name: [word arrays]}.
        B8.0   i8 across the sign        B8.1   5 distinct values (ties)
        B16.0  i16 across the sign       B16.1  u16 spread            B16.2  3 distinct values
        B32.0  f32 bits: the specials, then floats of both signs (the world's system adds 1 to the BITS every frame: still a key)      B32.1  i32 across the sign
        B64.0  f64 bits: the specials, then doubles of both signs     B64.1  u64 / i64: pairs that differ only in the high half or only in the low half"""
    i = np.arange(first, first + n, dtype=np.int64)
    rng = np.random.default_rng([77, first, n])
    f32 = rng.standard_normal(n).astype(np.float32).view(U32)
    f32[::7] = F32_SPECIALS[(i[::7] // 7) % F32_SPECIALS.size]
    f64 = rng.standard_normal(n).astype(np.float64).view(U64)
    f64[::5] = F64_SPECIALS[(i[::5] // 5) % F64_SPECIALS.size]
    hi, lo = (rng.integers(0, 4, n).astype(U64) << U64(62)), rng.integers(0, 3, n).astype(U64)
    return {"B8": [((i * 37 + 100) & 0xFF).astype(U8), (i * 3 % 5).astype(U8)],
            "B16": [((i * 4099 + 30000) & 0xFFFF).astype(U16), rng.integers(0, 1 << 16, n).astype(U16), (i % 3).astype(U16)],
            "B32": [f32, (rng.integers(-(1 << 31), 1 << 31, n)).astype(np.int32).view(U32)],
            "B64": [f64, np.where(i % 2 == 0, hi | U64(5), (U64(1) << U64(40)) | lo)]}


def spawn_planted(w, ids, n, first=0):
    if n == 0: return
    cols = planted_columns(n, first)
    w.spawn(n, {ids[name]: words for name, words in cols.items()})
