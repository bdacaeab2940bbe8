"""The state-diff tests' shared pieces (ggrs_hip_diff_frames / ggrs_hip_diff_block / ggrs_hip_snapshot_copy; include/ggrs_hip.h "STATE DIFF").

    model_diff      the semantics restated in numpy over plain arrays -- alive, presence, words per side -- with no knowledge of blocks, tiles or kernels
    build_schema    one world with every word width: Flag{u8}, Tag{u16}, Pos{x, y: u32}, Big{u64}, Quiet{u32, under no checksum}, Side{u32, NOT rollback:
                    must be ignored} and the device resource Clock{ticks, seed: u32}.  Its two systems do nothing in a frame whose input is 0:
                        bump   (entity system)     Pos.x += 3 * input; Big += input << 33
                        tick   (resource system)   Clock.ticks += input
    record          the live world's arrays through the existing download calls: call it where the live world IS the frame being saved
(A helper module, no tests of its own.)"""
import numpy as np

import bevy_ggrs_amd as bg

U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
NO_WORD = 0xFFFFFFFF

BUMP_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) { e.u32(0) += 3u * (ggrs_u32)f.input[0]; e.u64(1) += (ggrs_u64)f.input[0] << 33; }"
TICK_SRC = "__device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame& f) { r.u32(0) += (ggrs_u32)f.input[0]; }"


# ---------------------------------------------------------------------------------------------------------------- the model
def _pad(a, n, dtype=None):
    a = np.asarray(a) if dtype is None else np.asarray(a, dtype=dtype)
    if a.size >= n: return a[:n]
    return np.concatenate([a, np.zeros(n - a.size, dtype=a.dtype)])


def model_diff(A, B, comps, max_entries=64):
    """A, B: {"len": int, "alive": bool[len], "present": {comp: bool[len]}, "words": {(comp, word): uint[len]}, "res": {res: [ints]}}.
    comps: [(comp id, first column number, number of words)] of the ROLLBACK components, in id order.
    Returns {"len_a", "len_b", "n_entities", "n_alive", "n_presence": {comp: n}, "n_value": {comp: n}, "resource_diff": [res ..], "entries": [tuple ..]} with one
    tuple (slot, alive_a, alive_b, presence_diff, column_diff, first_comp, first_word, first_a, first_b) per differing entity: the max_entries lowest slots, ascending."""
    n = max(A["len"], B["len"])
    # a slot at or beyond a side's len is dead on that side
    aa = _pad(A["alive"], A["len"], bool); aa = _pad(aa, n); ab = _pad(B["alive"], B["len"], bool); ab = _pad(ab, n)
    both = aa & ab
    alive_x = aa ^ ab
    pres_bits = np.zeros(n, dtype=object); col_bits = np.zeros(n, dtype=object)
    pres_bits[:] = 0; col_bits[:] = 0
    first = {}                                                      # slot -> (comp, word, a, b) of the lowest differing column
    n_presence, n_value = {}, {}
    anyd = alive_x.copy()
    for c, col0, nw in comps:
        pa, pb = _pad(A["present"][c], n, bool), _pad(B["present"][c], n, bool)
        pd = (pa ^ pb) & both                                       # where the alive bits differ, nothing else is said
        common = pa & pb & both                                     # a component absent on either side has no words to compare
        vd = np.zeros(n, dtype=bool)
        for k in range(nw):
            wa, wb = _pad(A["words"][(c, k)], n), _pad(B["words"][(c, k)], n)
            assert wa.dtype == wb.dtype and wa.dtype.kind == "u", "words are compared as bits: hand them over as unsigned integers"
            ne = (wa != wb) & common
            for s in np.flatnonzero(ne):
                if not col_bits[s]: first[int(s)] = (c, k, int(wa[s]), int(wb[s]))
                col_bits[s] |= 1 << (col0 + k)
            vd |= ne
        for s in np.flatnonzero(pd): pres_bits[s] |= 1 << c
        if pd.any(): n_presence[c] = int(pd.sum())
        if vd.any(): n_value[c] = int(vd.sum())
        anyd |= pd | vd
    slots = np.flatnonzero(anyd)
    entries = []
    for s in slots[:max_entries]:
        s = int(s)
        fc, fw, fa, fb = first.get(s, (NO_WORD, NO_WORD, 0, 0))
        entries.append((s, int(aa[s]), int(ab[s]), int(pres_bits[s]), int(col_bits[s]), fc, fw, fa, fb))
    res = sorted(r for r in A.get("res", {}) if list(A["res"][r]) != list(B["res"][r]))
    return {"len_a": A["len"], "len_b": B["len"], "n_entities": int(slots.size), "n_alive": int(alive_x.sum()), "n_presence": n_presence, "n_value": n_value,
            "resource_diff": res, "entries": entries}


def as_model(d):
    """A bevy_ggrs_amd.StateDiff in the model's form."""
    mask = lambda bits: sum(1 << b for b in bits)
    entries = [(e.slot, int(e.alive_a), int(e.alive_b), mask(e.presence_diff), mask(e.column_diff), NO_WORD if e.first_comp is None else e.first_comp,
                NO_WORD if e.first_word is None else e.first_word, e.first_a, e.first_b) for e in d.entries]
    return {"len_a": d.len_a, "len_b": d.len_b, "n_entities": d.n_entities, "n_alive": d.n_alive, "n_presence": dict(d.n_presence), "n_value": dict(d.n_value),
            "resource_diff": list(d.resource_diff), "entries": entries}


# ---------------------------------------------------------------------------------------------------------------- the world
class Schema:
    """Component and resource ids of build_schema's world, the rollback components as model_diff wants them, and the word types."""

    def __init__(self): self.ids, self.shape, self.rollback, self.clock = {}, {}, [], None

    @property
    def comps(self):
        out, col = [], 0
        for name, (wb, nw) in self.shape.items():
            if name in self.rollback: out.append((self.ids[name], col, nw))
            col += nw                                               # (a non-rollback component's words are columns too: they take numbers)
        return out


def build_schema(w, *, with_side=True, with_resource=True):
    s = Schema()
    for name, wb, nw, rollback in (("Flag", 1, 1, True), ("Tag", 2, 1, True), ("Pos", 4, 2, True), ("Big", 8, 1, True), ("Quiet", 4, 1, True), ("Side", 4, 1, False)):
        if name == "Side" and not with_side: continue
        s.ids[name] = w.register_component(name, wb, nw, rollback=rollback); s.shape[name] = (wb, nw)
        if rollback: s.rollback.append(name)
    for name, words in (("Flag", [0]), ("Tag", [0]), ("Pos", [0, 1]), ("Big", [0])): w.checksum_component(s.ids[name], words)      # Quiet: under no checksum
    if with_resource:
        s.clock = w.register_resource("Clock", 4, 2, (5, 77)); w.checksum_resource(s.clock, [0, 1])
    w.add_custom_system(BUMP_SRC, [(s.ids["Pos"], 0), (s.ids["Big"], 0)], name="bump")
    if with_resource: w.add_resource_system(TICK_SRC, [(s.clock, 0)], name="tick")
    return s


def spawn_schema(w, s, n):
    """n entities; every 5th lacks Quiet, every 7th lacks Tag (components absent from the start)."""
    i = np.arange(n, dtype=np.int64)
    cols = {s.ids["Flag"]: [(i % 3).astype(U8)], s.ids["Tag"]: [(i * 11 % 65521).astype(U16)], s.ids["Pos"]: [(i * 7).astype(U32), (i ^ 0x5A5A).astype(U32)],
            s.ids["Big"]: [(i.astype(U64) << U64(34)) + U64(9)], s.ids["Quiet"]: [(i * 13 + 1).astype(U32)]}
    if "Side" in s.ids: cols[s.ids["Side"]] = [(i + 100).astype(U32)]
    w.spawn(n, cols)
    for k in range(0, n, 5): w.remove_component(s.ids["Quiet"], k)
    for k in range(0, n, 7): w.remove_component(s.ids["Tag"], k)


def record(w, s):
    """The live world's arrays through the download calls (alive, presence and words of the rollback components, the resource's words)."""
    n = w.len
    rec = {"len": n, "alive": w.alive_mask(n), "present": {}, "words": {}, "res": {}}
    for name in s.rollback:
        c = s.ids[name]
        rec["present"][c] = w.present_mask(c, n)
        for k in range(s.shape[name][1]): rec["words"][(c, k)] = w.download_word(c, k, 0, n)
    if s.clock is not None: rec["res"][s.clock] = w.resource_read(s.clock)
    return rec


def adv(inp=1): return bg.AdvanceFrame((inp,))
