"""The checksum-parts tests' shared pieces (ggrs_hip_checksum_parts / ggrs_hip_checksum_parts_block; include/ggrs_hip.h "CHECKSUM PARTS").

    model_parts     the semantics restated in numpy over plain arrays -- len, alive, presence, words, resource words -- from the oracle's numpy pieces
                    (oracle.oracle_np: np_inner_hash_fields, np_entity_part, SeaHasher, entity_checksum), with no knowledge of blocks, tiles or kernels
    Specs           a world's checksum registrations as the model wants them
    schema_specs    ... of state_diff_common.build_schema's world
    record_words    the live world's arrays through the download calls, for any backend world and any list of components
(A helper module, no tests of its own.)"""
from collections import OrderedDict
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle_np as onp

U64 = np.uint64
M64 = (1 << 64) - 1


@dataclass
class Specs:
    """components: [(name, component id, fields)] in id order, fields = [(word index, bytes the word contributes)] or a callable
    hasher(words: {word index: column of the hashed entities}, slots) -> uint64 column (a user-written hasher restated in numpy).
    resources: [(name, resource id, word bytes, [word index ..])] in id order, the checksummed ones only."""
    components: list = field(default_factory=list)
    resources: list = field(default_factory=list)


def sea_one(x):
    return onp.SeaHasher().write_u64(x).finish()


def _fit(a, n, dtype=None):
    a = np.asarray(a) if dtype is None else np.asarray(a, dtype=dtype)
    if a.size >= n: return a[:n]
    return np.concatenate([a, np.zeros(n - a.size, dtype=a.dtype)])


def model_parts(rec, specs):
    """rec: {"len": int, "alive": bool[..], "present": {comp: bool[..]}, "words": {(comp, word): uint[..]}, "res": {res: [ints]}} (state_diff_common.record).
    Returns {"parts": name -> value (ordered: components, "Entity", resources), "counts": name -> n_hashed, "len", "active", "checksum"}."""
    n = int(rec["len"])
    alive = _fit(rec["alive"], n, bool)                                # a slot at or beyond len is dead whatever its mask bit says
    parts, counts = OrderedDict(), {}
    for name, c, fields in specs.components:
        sel = alive & _fit(rec["present"][c], n, bool)
        slots = np.flatnonzero(sel).astype(U64)                        # RollbackOrdered::order == slot
        x = 0
        if slots.size:
            if callable(fields):
                nw = 1 + max(k for (cc, k) in rec["words"] if cc == c)
                inner = np.asarray(fields({k: _fit(rec["words"][(c, k)], n)[sel] for k in range(nw)}, slots), dtype=U64)
            else:
                assert fields, "a word-list spec names at least one word"
                inner = onp.np_inner_hash_fields([(_fit(rec["words"][(c, k)], n)[sel], nb) for k, nb in fields])
            x = int(np.bitwise_xor.reduce(onp.np_entity_part(slots, inner)))
        parts[name] = sea_one(x)                                       # nobody holds it: sea_one(0), not 0
        counts[name] = int(slots.size)
    active = int(alive.sum())
    parts["Entity"] = onp.entity_checksum(active, n)
    counts["Entity"] = active
    for name, r, wb, words in specs.resources:
        h = onp.SeaHasher()
        for k in words: h.write((int(rec["res"][r][k]) & ((1 << (8 * wb)) - 1)).to_bytes(wb, "little"))
        parts[name] = h.finish()
        counts[name] = 0
    total = 0
    for v in parts.values(): total ^= v
    return {"parts": parts, "counts": counts, "len": n, "active": active, "checksum": total}


def as_model(p):
    """A bevy_ggrs_amd.ChecksumParts in the model's form."""
    return {"parts": OrderedDict(p.parts), "counts": dict(p.counts), "len": p.len, "active": p.active, "checksum": p.checksum}


def schema_specs(s):
    """state_diff_common.build_schema: Flag{u8}, Tag{u16}, Pos{x, y: u32}, Big{u64} are checksummed (Quiet and Side are not), and the resource Clock{ticks, seed}."""
    comps = [(name, s.ids[name], [(k, s.shape[name][0]) for k in range(s.shape[name][1])]) for name in ("Flag", "Tag", "Pos", "Big")]
    return Specs(sorted(comps, key=lambda t: t[1]), [("Clock", s.clock, 4, [0, 1])] if s.clock is not None else [])


def record_words(w, comps, res=()):
    """The live world of any backend as a rec: comps = [(component id, number of words)], res = [resource id ..]."""
    n = w.len
    rec = {"len": n, "alive": w.alive_mask(n), "present": {}, "words": {}, "res": {}}
    for c, nw in comps:
        rec["present"][c] = w.present_mask(c, n)
        for k in range(nw): rec["words"][(c, k)] = w.download_word(c, k, 0, n)
    for r in res: rec["res"][r] = w.resource_read(r)
    return rec
