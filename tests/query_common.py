"""The query tests' shared pieces (ggrs_hip_query_layout / ggrs_hip_query / ggrs_hip_query_block; include/ggrs_hip.h "QUERY").

    model_query      the semantics restated in numpy over plain arrays -- alive, presence, words -- with no knowledge of blocks, tiles or kernels
    expected_buffer  the model's rows laid out as the header says the one output buffer is (256-byte aligned column starts, desc order, slots last), over a
                     buffer pre-filled with FILL: what the device's buffer must equal byte for byte, padding and the rows beyond n_rows included
    record           a world's live state through the download calls (download_alive / download_present / download_word: the route a host takes today)
    device_query     World.query into a buffer pre-filled with FILL, as (n_matched, n_rows, bytes)
    build_widths     one world with every word width and a filter-only component:
                         B8 {2 x u8}, B16 {3 x u16}, B32 {2 x u32}, B64 {2 x u64}, Mark {1 x u32}; its one system adds 1 to B32.0 every frame
(A helper module, no tests of its own.)"""
import numpy as np

import bevy_ggrs_amd as bg

U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
UINT = {1: U8, 2: U16, 4: U32, 8: U64}
FILL = 0xA5
ALIGN = 256


# ---------------------------------------------------------------------------------------------------------------- the model
def as_bits(mask, n):
    """A mask as bool[n]: from bools, or from the uint64 words the C ABI's download calls fill (bit i of word k is slot 64 k + i); short masks are padded with 0."""
    m = np.asarray(mask)
    if m.dtype == np.uint64: m = np.unpackbits(m.view(np.uint8), bitorder="little")
    m = m.astype(bool)[:n]
    return np.concatenate([m, np.zeros(n - m.size, dtype=bool)]) if m.size < n else m


def make_desc(fetch=(), with_=(), without=(), slots=True):
    """fetch: (comp, word) pairs."""
    return {"fetch": [tuple(f) for f in fetch], "with": set(with_), "without": set(without), "slots": bool(slots)}


def model_query(alive_words, len_, present_words_by_comp, columns, desc, max_rows):
    """alive_words, present_words_by_comp[c]: masks (bool arrays or uint64 words) that may be longer than len_; columns[(c, w)]: an unsigned array of at least
    len_ words.  Slot s matches iff s < len_, it is alive, it has every With component and every fetched word's component, and it has no Without component.
    Rows are the matching slots, ascending; n_matched is exact, the first min(n_matched, max_rows) rows are returned."""
    match = as_bits(alive_words, len_)
    for c in sorted(desc["with"] | {c for c, _ in desc["fetch"]}): match = match & as_bits(present_words_by_comp[c], len_)
    for c in sorted(desc["without"]): match = match & ~as_bits(present_words_by_comp[c], len_)
    slots = np.flatnonzero(match)
    n_rows = min(int(slots.size), int(max_rows))
    rows = slots[:n_rows]
    cols = []
    for key in desc["fetch"]:
        col = np.asarray(columns[key])
        assert col.dtype.kind == "u", "words are bits: hand them over as unsigned integers"
        cols.append(col[rows].copy())
    return {"n_matched": int(slots.size), "n_rows": n_rows, "slots": rows.astype(U32) if desc["slots"] else None, "columns": cols}


def align_up(x, a=ALIGN): return (x + a - 1) // a * a


def model_layout(word_bytes, slots, max_rows):
    """(column offsets, slots offset or None, total bytes) of the one output buffer, restated from the header."""
    off, offs = 0, []
    for wb in word_bytes:
        offs.append(off); off = align_up(off + max_rows * wb)
    s_off = None
    if slots: s_off = off; off = align_up(off + max_rows * 4)
    return offs, s_off, off


def expected_buffer(res, word_bytes, max_rows, size):
    """The bytes of an output buffer of `size` bytes pre-filled with FILL after the query whose model result is `res`."""
    offs, s_off, total = model_layout(word_bytes, res["slots"] is not None, max_rows)
    assert size >= total
    buf = np.full(size, FILL, dtype=U8)
    for off, wb, col in zip(offs, word_bytes, res["columns"]):
        assert col.dtype.itemsize == wb
        buf[off:off + col.size * wb] = col.view(U8)
    if s_off is not None: buf[s_off:s_off + res["slots"].size * 4] = res["slots"].view(U8)
    return buf


# ---------------------------------------------------------------------------------------------------------------- the device
def record(w, comps=None):
    """The live world's alive mask, presence masks and words of `comps` (default: every component) through the download calls."""
    n = w.len
    comps = range(len(w._comps)) if comps is None else comps
    rec = {"len": n, "alive": w.alive_mask(n), "present": {}, "columns": {}}
    for c in comps:
        rec["present"][c] = w.present_mask(c, n)
        for k in range(w._comps[c][2]): rec["columns"][(c, k)] = w.download_word(c, k, 0, n)
    return rec


def model_of(rec, desc, max_rows): return model_query(rec["alive"], rec["len"], rec["present"], rec["columns"], desc, max_rows)


def word_bytes_of(w, desc): return [w._comps[c][1] for c, _ in desc["fetch"]]


def device_query(w, state, desc, max_rows, extra=512):
    """World.query into a buffer pre-filled with FILL (`extra` bytes longer than the layout asks for): (n_matched, n_rows, the whole buffer's bytes)."""
    import torch
    _, _, total = model_layout(word_bytes_of(w, desc), desc["slots"], max_rows)
    out = torch.full((total + extra,), FILL, dtype=torch.uint8, device=f"cuda:{w.device}")
    r = w.query(state, desc["fetch"], with_=desc["with"], without=desc["without"], slots=desc["slots"], max_rows=max_rows, out=out)
    assert r.buffer is out and r.n_rows == min(r.n_matched, max_rows)
    return r.n_matched, r.n_rows, out.cpu().numpy()


def assert_query_equals_model(w, state, rec, desc, max_rows, ctx=""):
    """The device's buffer against the model's, bit for bit (rows, the bytes beyond them and the padding); returns the model's result."""
    want = model_of(rec, desc, max_rows)
    n_matched, n_rows, buf = device_query(w, state, desc, max_rows)
    assert (n_matched, n_rows) == (want["n_matched"], want["n_rows"]), (ctx, n_matched, n_rows, want["n_matched"], want["n_rows"])
    exp = expected_buffer(want, word_bytes_of(w, desc), max_rows, buf.size)
    if not np.array_equal(buf, exp):
        bad = np.flatnonzero(buf != exp)
        raise AssertionError(f"{ctx}: output buffer differs from the model at {bad.size} bytes, first at {bad[:8]}: {buf[bad[:8]]} vs {exp[bad[:8]]}")
    return want


# ---------------------------------------------------------------------------------------------------------------- the worlds
WIDTHS = (("B8", 1, 2), ("B16", 2, 3), ("B32", 4, 2), ("B64", 8, 2), ("Mark", 4, 1))


def build_widths(w):
    """Registers WIDTHS and one system (B32.0 += 1 per frame); returns {name: id}."""
    ids = {name: w.register_component(name, wb, nw) for name, wb, nw in WIDTHS}
    for name, _, nw in WIDTHS: w.checksum_component(ids[name], list(range(nw)))
    w.add_system(bg.SYS_ADD_U32, comp=(ids["B32"],), word=(0,), iparam=(1,))
    return ids


def spawn_widths(w, ids, n, first=0):
    """n entities whose every word says which slot, component and word it is; Mark is absent (insert it where a test wants it)."""
    if n == 0: return
    i = np.arange(first, first + n, dtype=np.int64)
    w.spawn(n, {ids["B8"]: [((i * 3 + k) & 0xFF).astype(U8) for k in range(2)], ids["B16"]: [((i * 7 + 1000 * k) & 0xFFFF).astype(U16) for k in range(3)],
                ids["B32"]: [(i * 11 + (k << 28)).astype(U32) for k in range(2)], ids["B64"]: [(i.astype(U64) << U64(33)) + U64(5 + k) for k in range(2)]})


def all_words(w, ids, names): return [(ids[nm], k) for nm in names for k in range(w._comps[ids[nm]][2])]


# ---------------------------------------------------------------------------------------------------------------- the fuzz: a plan and its numpy shadow
FUZZ_SEEDS = 24
FUZZ_CAPACITY = 2048
MASK = {1: 0xFF, 2: 0xFFFF, 4: 0xFFFFFFFF, 8: 0xFFFFFFFFFFFFFFFF}


def fuzz_value(slot, comp, word, salt, wb):
    """What the plan writes into word `word` of component `comp` of slot `slot` (numpy int arrays or ints): a function of where it is."""
    with np.errstate(over="ignore"):                                            # (arithmetic modulo 2^64 is what is meant)
        v = (np.atleast_1d(np.asarray(slot, dtype=U64)) * U64(0x9E3779B97F4A7C15) + U64(comp * 1000003 + word * 7919 + salt * 104729 + 1)) * U64(0xD6E8FEB86659FD93)
    return ((v >> U64(13)) & U64(MASK[wb])).astype(UINT[wb])


class Shadow:
    """The fuzz world restated in numpy: alive, presence and words of every slot, under the plan's operations and the world's one system (component 0, word 0:
    a u32 that grows by 1 per frame where the entity is alive and has it)."""

    def __init__(self, comps):
        self.comps, self.len = comps, 0
        self.alive = np.zeros(FUZZ_CAPACITY, dtype=bool)
        self.present = {c: np.zeros(FUZZ_CAPACITY, dtype=bool) for c in range(len(comps))}
        self.columns = {(c, k): np.zeros(FUZZ_CAPACITY, dtype=UINT[wb]) for c, (_, wb, nw) in enumerate(comps) for k in range(nw)}

    def apply(self, op):
        if op[0] == "spawn":
            _, count, which, salt = op
            s = np.arange(self.len, self.len + count)
            self.alive[s] = True
            for c in range(len(self.comps)):
                self.present[c][s] = c in which
                if c in which:
                    for k in range(self.comps[c][2]): self.columns[(c, k)][s] = fuzz_value(s, c, k, salt, self.comps[c][1])
            self.len += count
        elif op[0] == "despawn": self.alive[op[1]] = False
        elif op[0] == "remove": self.present[op[1]][op[2]] = False
        elif op[0] == "insert":
            _, c, s, salt = op
            self.present[c][s] = True
            for k in range(self.comps[c][2]): self.columns[(c, k)][s] = fuzz_value(s, c, k, salt, self.comps[c][1])[0]
        elif op[0] == "tick":
            on = self.alive & self.present[0]
            self.columns[(0, 0)][on] += U32(1)

    def rec(self):
        n = self.len
        return {"len": n, "alive": self.alive[:n].copy(), "present": {c: p[:n].copy() for c, p in self.present.items()}, "columns": {k: v[:n].copy() for k, v in self.columns.items()}}


def fuzz_plan(seed):
    """(components, operations before Save(0), operations between Save(0) and the ticks, descs) of one seed: pure CPU, the same on every machine.  A desc is
    (make_desc(..), max_rows or None for len)."""
    rng = np.random.default_rng([2026, seed])
    comps = [("Tick", 4, 1)] + [(f"C{i}", int(rng.choice([1, 2, 4, 8])), int(rng.integers(1, 4))) for i in range(1, int(rng.integers(2, 6)))]
    nc = len(comps)
    sh = Shadow(comps)                                                          # (only to know who is alive while the plan is drawn)

    def subset(p): return {c for c in range(nc) if rng.random() < p}

    def edits(k):
        ops = []
        for _ in range(k):
            live = np.flatnonzero(sh.alive[:sh.len])
            if live.size == 0: break
            s, c, kind = int(rng.choice(live)), int(rng.integers(0, nc)), rng.random()
            op = ("despawn", s) if kind < 0.4 else ("remove", c, s) if kind < 0.7 else ("insert", c, s, int(rng.integers(1, 1000)))
            sh.apply(op); ops.append(op)
        return ops

    def spawn(count):
        which = subset(0.7)
        if rng.random() < 0.5 or not which: which |= {0}                        # (never a bundle of nothing)
        op = ("spawn", count, which, int(rng.integers(1, 1000)))
        sh.apply(op); return op

    n0 = int(rng.choice([1, 40, 64, 65, 130, 500, 700]))
    before = [spawn(n0)] + edits(int(rng.integers(0, 60)))
    between = [spawn(int(rng.integers(1, 200)))] + edits(int(rng.integers(0, 60)))
    descs = []
    for _ in range(4):
        fetch = []
        for _k in range(int(rng.integers(0, 5))):
            c = int(rng.integers(0, nc)); fetch.append((c, int(rng.integers(0, comps[c][2]))))
        with_ = subset(0.25)
        without = subset(0.3) - with_ - {c for c, _ in fetch}
        cap = [None, 0, 1, 5, 37, 200][int(rng.integers(0, 6))]
        descs.append((make_desc(fetch, with_, without, slots=bool(rng.random() < 0.7) or not fetch), cap))
    return comps, before, between, descs


def fuzz_shadow_states(seed):
    """(comps, the shadow's record at Save(0), its record of the live world after the ticks, descs) of one seed."""
    comps, before, between, descs = fuzz_plan(seed)
    sh = Shadow(comps)
    for op in before: sh.apply(op)
    rec0 = sh.rec()
    for op in between: sh.apply(op)
    sh.apply(("tick",)); sh.apply(("tick",))
    return comps, rec0, sh.rec(), descs


def fuzz_coverage(seed):
    """What one seed exercises, from the model over the shadow: the word widths fetched, With, Without, a truncated result, an empty one."""
    comps, rec0, live, descs = fuzz_shadow_states(seed)
    hit = set()
    for rec in (rec0, live):
        for desc, cap in descs:
            r = model_of(rec, desc, rec["len"] if cap is None else cap)
            hit |= {f"width{comps[c][1]}" for c, _ in desc["fetch"]}
            if desc["with"]: hit.add("with")
            if desc["without"]: hit.add("without")
            if r["n_rows"] < r["n_matched"]: hit.add("truncated")
            if r["n_matched"] == 0: hit.add("empty")
            if r["n_matched"] > 64: hit.add("many_units")
    return hit


FUZZ_FLOORS = ("width1", "width2", "width4", "width8", "with", "without", "truncated", "empty", "many_units")
