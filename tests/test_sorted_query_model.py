"""The sorted query without a GPU: the numpy restatement (sorted_query_common.model_query_sorted) held to hand-written cases whose expected order is written out,
not computed; the proof that those cases can SEE a wrong order: three deliberately wrong models -- ties broken by descending slot under DESC, F ordered as signed
integers, the halves of an 8-byte key swapped -- must each fail one of them; every refusal and its message on a layout-only world (the descs are judged before
the device is looked at); and the new kernels' own text run on the host against std::stable_sort (tests/cpp/sort_host_emulation.cpp).

The hand-written cases, the layout case and the wrong-model cases hold the MODEL, not the library: they say what the yardstick of every device test is worth and
need no entry point, so they pass wherever sorted_query_common.py exists.  The refusals and the host emulation run the library's own code."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import query_common as qc
import sorted_query_common as sq
from bevy_ggrs_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64


def rec_of(columns, alive=None, present=None):
    """A record of len(column) slots, all alive and all present unless told otherwise; columns: {(comp, word): array}."""
    n = len(next(iter(columns.values())))
    comps = {c for c, _ in columns}
    return {"len": n, "alive": np.ones(n, dtype=bool) if alive is None else np.asarray(alive, dtype=bool),
            "present": {c: np.ones(n, dtype=bool) if present is None or c not in present else np.asarray(present[c], dtype=bool) for c in comps}, "columns": columns}


def order_of(model, columns, order_by, max_rows=None, **kw):
    rec = rec_of(columns, **kw)
    return model(rec, qc.make_desc([]), order_by, rec["len"] if max_rows is None else max_rows)["slots"].tolist()


def f32(*xs): return np.array(xs, dtype=np.float32).view(U32)
def f64(*xs): return np.array(xs, dtype=np.float64).view(U64)


# the hand-written total order: -NaN, -inf, -1.0, -denormal, -0.0, +0.0, +denormal, 1.0, +inf, +NaN
F32_ORDERED = np.array([0xFFC00000, 0xFF800000, 0xBF800000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x3F800000, 0x7F800000, 0x7FC00000], dtype=U32)
F64_ORDERED = np.array([0xFFF8000000000000, 0xFFF0000000000000, 0xBFF0000000000000, 0x8000000000000001, 0x8000000000000000,
                        0x0000000000000000, 0x0000000000000001, 0x3FF0000000000000, 0x7FF0000000000000, 0x7FF8000000000000], dtype=U64)
SHUFFLE = [7, 2, 9, 0, 5, 3, 8, 1, 6, 4]                    # slot s holds ORDERED[SHUFFLE[s]]
SHUFFLE_SORTED = [3, 7, 1, 5, 9, 4, 8, 0, 6, 2]             # the slot that holds ORDERED[k], k = 0 .. 9 (written out: SHUFFLE's inverse)
HALVES = np.array([0x0000000200000001, 0x0000000100000003, 0x0000000100000002, 0x0000000200000000], dtype=U64)       # differ in the high half AND the other way in the low half


def hand_written_cases(model):
    """Every case as (what, got, expected): the expected orders are literals."""
    out = []
    assert [SHUFFLE[s] for s in SHUFFLE_SORTED] == list(range(10))
    out.append(("f32 total order", order_of(model, {(0, 0): F32_ORDERED[SHUFFLE]}, [(0, 0, "f")]), SHUFFLE_SORTED))
    out.append(("f64 total order", order_of(model, {(0, 0): F64_ORDERED[SHUFFLE]}, [(0, 0, "f")]), SHUFFLE_SORTED))
    out.append(("f32 total order, desc", order_of(model, {(0, 0): F32_ORDERED[SHUFFLE]}, [(0, 0, "f", "desc")]), SHUFFLE_SORTED[::-1]))
    out.append(("NaN payloads", order_of(model, {(0, 0): np.array([0x7FC00002, 0xFFC00002, 0x7FC00001, 0xFFC00001], dtype=U32)}, [(0, 0, "f")]), [1, 3, 2, 0]))
    # integers across the sign: slots hold 1, -1, 0, min, max
    for wb, dt in ((1, np.int8), (2, np.int16), (4, np.int32), (8, np.int64)):
        info = np.iinfo(dt)
        col = np.array([1, -1, 0, info.min, info.max], dtype=dt).view(qc.UINT[wb])
        out.append((f"i{8 * wb} across the sign", order_of(model, {(0, 0): col}, [(0, 0, "i")]), [3, 1, 2, 0, 4]))
        out.append((f"u{8 * wb}: the same bits unsigned", order_of(model, {(0, 0): col}, [(0, 0, "u")]), [2, 0, 4, 3, 1]))
    out.append(("u64 differing only in the high half", order_of(model, {(0, 0): np.array([3 << 32, 1 << 32, 2 << 32], dtype=U64) | U64(7)}, [(0, 0, "u")]), [1, 2, 0]))
    out.append(("u64 differing only in the low half", order_of(model, {(0, 0): np.array([3, 1, 2], dtype=U64) | U64(9 << 32)}, [(0, 0, "u")]), [1, 2, 0]))
    out.append(("u64: the high half decides over the low half", order_of(model, {(0, 0): HALVES}, [(0, 0, "u")]), [2, 1, 3, 0]))
    ties = np.array([5, 3, 5, 3, 5, 9], dtype=U32)
    out.append(("ties keep ascending slots", order_of(model, {(0, 0): ties}, [(0, 0, "u")]), [1, 3, 0, 2, 4, 5]))
    out.append(("ties under desc keep ascending slots", order_of(model, {(0, 0): ties}, [(0, 0, "u", "desc")]), [5, 0, 2, 4, 1, 3]))
    two = {(0, 0): np.array([1, 0, 1, 0, 1], dtype=U8), (1, 0): np.array([30, 20, 10, 20, 30], dtype=U16)}
    out.append(("two keys: keys[0] is the most significant", order_of(model, two, [(0, 0, "u"), (1, 0, "u")]), [1, 3, 2, 0, 4]))
    out.append(("two keys the other way round", order_of(model, two, [(1, 0, "u"), (0, 0, "u")]), [2, 1, 3, 0, 4]))
    out.append(("two keys, the second desc", order_of(model, two, [(0, 0, "u"), (1, 0, "u", "desc")]), [1, 3, 0, 4, 2]))
    four = {(0, 0): np.array([0, 0, 0, 0, 0, 1], dtype=U8), (0, 1): np.array([2, 2, 2, 2, 1, 0], dtype=U8),
            (1, 0): np.array([7, 7, 7, 6, 9, 0], dtype=U32), (2, 0): np.array([5, 4, 5, 9, 9, 0], dtype=U64)}
    out.append(("four keys", order_of(model, four, [(0, 0, "u"), (0, 1, "u"), (1, 0, "u"), (2, 0, "u")]), [4, 3, 1, 0, 2, 5]))
    out.append(("top-k: the first rows of the full order", order_of(model, {(0, 0): ties}, [(0, 0, "u", "desc")], max_rows=2), [5, 0]))
    out.append(("a key's component counts as With", order_of(model, {(0, 0): ties}, [(0, 0, "u")], present={0: [1, 0, 1, 1, 1, 1]}), [3, 0, 2, 4, 5]))
    out.append(("the dead do not match", order_of(model, {(0, 0): ties}, [(0, 0, "u")], alive=[1, 1, 0, 1, 1, 0]), [1, 3, 0, 4]))
    return out


def test_the_model_on_hand_written_cases():
    for what, got, want in hand_written_cases(sq.model_query_sorted): assert got == want, what


def test_the_model_returns_the_querys_rows_and_layout():
    rec = rec_of({(0, 0): np.array([4, 1, 3, 1], dtype=U16), (1, 0): np.arange(4, dtype=U64) * U64(10)})
    desc = qc.make_desc([(1, 0), (0, 0)])
    r = sq.model_query_sorted(rec, desc, [(0, 0, "u")], 3)
    assert (r["n_matched"], r["n_rows"]) == (4, 3) and r["slots"].tolist() == [1, 3, 2] and r["columns"][0].tolist() == [10, 30, 20] and r["columns"][1].tolist() == [1, 1, 3]
    assert sorted(r["slots"].tolist() + [0]) == qc.model_of(rec, desc, 4)["slots"].tolist()                    # the same rows as the query
    buf = sq.expected_buffer(r, [8, 2], 3, 1024)
    assert buf[24] == qc.FILL and buf[256:262].view(U16).tolist() == [1, 1, 3] and buf[512:524].view(U32).tolist() == [1, 3, 2]
    assert sq.model_query_sorted(rec, desc, [(0, 0, "u")], 0)["n_matched"] == 4                              # max_rows 0: a count


# ---------------------------------------------------------------------------------------------------------------- wrong models must be caught
def _wrong_desc_ties(rec, desc, order_by, max_rows):
    """DESC as the reversal of the ascending order: ties come out in DESCENDING slot order."""
    if not any(len(k) == 4 for k in order_by): return sq.model_query_sorted(rec, desc, order_by, max_rows)
    asc = sq.model_query_sorted(rec, qc.make_desc(desc["fetch"], desc["with"], desc["without"], True), [k[:3] for k in order_by], rec["len"])
    return {"n_matched": asc["n_matched"], "n_rows": min(asc["n_matched"], max_rows), "slots": asc["slots"][::-1][:max_rows], "columns": []}


def _wrong_f_as_signed(rec, desc, order_by, max_rows):
    return sq.model_query_sorted(rec, desc, [(k[0], k[1], "i" if k[2] == "f" else k[2]) + tuple(k[3:]) for k in order_by], max_rows)


def _wrong_halves_swapped(rec, desc, order_by, max_rows):
    cols = {k: (((v >> U64(32)) | (v << U64(32))) if v.dtype == U64 else v) for k, v in rec["columns"].items()}
    return sq.model_query_sorted(dict(rec, columns=cols), desc, order_by, max_rows)


@pytest.mark.parametrize("wrong, caught_by", [(_wrong_desc_ties, "ties under desc keep ascending slots"), (_wrong_f_as_signed, "f32 total order"),
                                              (_wrong_halves_swapped, "u64: the high half decides over the low half")],
                         ids=["desc_ties_by_descending_slot", "f_as_signed_integers", "halves_of_an_8_byte_key_swapped"])
def test_a_wrong_model_is_caught(wrong, caught_by):
    failed = [what for what, got, want in hand_written_cases(wrong) if got != want]
    assert caught_by in failed, failed


# ---------------------------------------------------------------------------------------------------------------- refusals: no device needed
STRATEGY_SRC = ("__device__ void ggrs_store(const GgrsWords& t, GgrsWords& s) { s.u16(0) = (unsigned short)t.u32(0); }\n"
                "__device__ void ggrs_load(const GgrsWords& s, GgrsWords& t) { t.u32(0) = s.u16(0); }")


def test_every_refusal_and_its_message_on_a_layout_only_world():
    w = bg.World(1000, max_depth=4, flags=bg.GGRS_WORLD_LAYOUT_ONLY)
    ids = qc.build_widths(w)
    St = w.register_component("Stored", 4, 1); w.register_component_strategy(St, 2, 1, STRATEGY_SRC)
    Nr = w.register_component("Plain", 4, 1, rollback=False)
    rep = _ffi.QueryReport()
    out = C.c_void_p(0x1000)                                                                       # never dereferenced: every call below is refused before the device
    fetch = w.query_desc([(ids["B8"], 0)])

    def refused(order_by, what, desc=fetch, state=bg.LIVE, code=bg.GGRS_E_INVALID, sdesc=None, block=False, out_ptr=out, max_rows=4):
        sd = w.sort_desc(order_by) if sdesc is None else sdesc
        if block: rc = w._lib.ggrs_hip_query_sorted_block(w._p, C.c_void_p(0x2000), C.byref(desc), C.byref(sd), out_ptr, max_rows, C.byref(rep))
        else: rc = w._lib.ggrs_hip_query_sorted(w._p, state, C.byref(desc), C.byref(sd), out_ptr, max_rows, C.byref(rep))
        msg = w._lib.ggrs_hip_last_error(w._p).decode()
        assert rc == code and all(x in msg for x in ([what] if isinstance(what, str) else what)), (rc, msg)

    key = [(ids["B32"], 0, "f")]
    # everything query_check refuses
    d = w.query_desc([(ids["B8"], 0)]); d.words[0].comp = 17
    refused(key, "component 17", desc=d)
    refused(key, "word 2 of component B8", desc=w.query_desc([(ids["B8"], 2)]))
    refused(key, "With", desc=w.query_desc([(ids["B32"], 0)], without=[ids["B32"]]))
    d = w.query_desc([]); d.flags = 2
    refused(key, "unknown query flags", desc=d)
    refused(key, "no output buffer", out_ptr=None)
    # the sort desc
    refused([], "use ggrs_hip_query")
    sd = w.sort_desc(key); sd.n_keys = 5
    refused(None, ["at most 4 keys", "5"], sdesc=sd)
    sd = w.sort_desc(key); sd.flags = 1
    refused(None, "unknown sort flags 0x1", sdesc=sd)
    sd = w.sort_desc(key + key); sd.keys[1].kind = 3
    refused(None, ["sort key 1", "unknown kind 0x3"], sdesc=sd)
    sd = w.sort_desc(key); sd.keys[0].kind = _ffi.SORT_F | 0x200
    refused(None, ["sort key 0", "unknown kind 0x202"], sdesc=sd)
    sd = w.sort_desc(key); sd.keys[0].comp = 29
    refused(None, ["sort key 0", "component 29"], sdesc=sd)
    refused([(ids["B8"], 0, "u"), (ids["B64"], 2, "u")], ["sort key 1", "word 2 of component B64"])
    refused([(ids["B8"], 0, "f")], ["sort key 0", "GGRS_SORT_F", "1-byte", "B8"])
    refused([(ids["B16"], 1, "f", "desc")], ["sort key 0", "GGRS_SORT_F", "2-byte", "B16"])
    refused([(ids["Mark"], 0, "u")], ["sort key 0", "Mark", "without_mask"], desc=w.query_desc([(ids["B8"], 0)], without=[ids["Mark"]]))
    for kw in ({"state": 2}, {"block": True}):                                                     # a ring frame, a block: Stored words, live-only components
        refused([(ids["B8"], 0, "u"), (St, 0, "u")], ["sort key 1", "Stored", "Strategy", "GGRS_DIFF_LIVE"], **kw)
        refused([(Nr, 0, "i")], ["sort key 0", "Plain", "not registered for rollback", "GGRS_DIFF_LIVE"], **kw)
        refused(key, "not registered for rollback", desc=w.query_desc([(ids["B8"], 0)], with_=[Nr]), **kw)      # what query_check_snapshot refuses
    # a good desc: the world has no device
    for order_by in (key, [(St, 0, "u")], [(Nr, 0, "i", "desc")], [(ids["B8"], 1, "i"), (ids["B16"], 0, "u"), (ids["B32"], 1, "f"), (ids["B64"], 0, "f", "desc")]):
        refused(order_by, "layout-only", code=bg.GGRS_E_NO_DEVICE)
    refused(key, "layout-only", code=bg.GGRS_E_NO_DEVICE, state=2)
    refused(key, "layout-only", code=bg.GGRS_E_NO_DEVICE, block=True)
    rc = w._lib.ggrs_hip_query_sorted_block(w._p, None, C.byref(fetch), C.byref(w.sort_desc(key)), out, 4, C.byref(rep))
    assert rc == bg.GGRS_E_INVALID and b"without a block" in w._lib.ggrs_hip_last_error(w._p)
    rc = w._lib.ggrs_hip_query_sorted(w._p, bg.LIVE, C.byref(fetch), None, out, 4, C.byref(rep))
    assert rc == bg.GGRS_E_INVALID and b"without a sort desc" in w._lib.ggrs_hip_last_error(w._p)
    # the Python layer's own checks
    with pytest.raises(ValueError): w.sort_desc([(0, 0, "x")])
    with pytest.raises(ValueError): w.sort_desc([(0, 0, "u", "asc")])
    with pytest.raises(ValueError): w.sort_desc([(0, 0, "u")] * 5)
    sd = w.sort_desc([(3, 1, "f", "desc"), (2, 0, "i")])
    assert (sd.n_keys, sd.flags, sd.keys[0].comp, sd.keys[0].word, sd.keys[0].kind, sd.keys[1].kind) == (2, 0, 3, 1, _ffi.SORT_F | _ffi.SORT_DESC, _ffi.SORT_I)
    assert C.sizeof(_ffi.SortDesc) == 56 and C.sizeof(_ffi.SortKey) == 12


# ---------------------------------------------------------------------------------------------------------------- the kernels' own text on the host
SORT_FIRST = "// ------------------------------------------------------------------ SORTED QUERY (ggrs_hip_query_sorted / ggrs_hip_query_sorted_block)"
SORT_LAST = "// ------------------------------------------------------------------ END OF SORTED QUERY"


def cut_sections():
    text = open(os.path.join(ROOT, "bevy_ggrs_amd", "csrc", "kernels.hpp")).read()
    ix = text[text.index("constexpr uint32_t IX_TPB = 256"):text.index("// THE INBOX (ggrs_hip_add_custom_system_effects")]
    sort = text[text.index(SORT_FIRST):text.index(SORT_LAST) + len(SORT_LAST)]
    return ix, sort


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_the_sort_kernels_own_text_run_on_the_host_equals_stable_sort(tmp_path):
    """k_sort_rows / k_sort_rekey / k_sort_small / k_sort_emit and the radix passes between them, as they stand in kernels.hpp, compiled for the host with one thread
    per lane: n_matched 1, 65, 2000, 2049 and 4100, both forms where n <= 2048, widths 1, 2, 4 and 8, two keys, DESC, a key with fewer than 8 distinct values;
    every array exactly sized."""
    ix, sort = cut_sections()
    assert all(k in sort for k in ("k_sort_rows", "k_sort_rekey", "k_sort_small", "k_sort_emit"))
    (tmp_path / "ix_kernels.inc").write_text(ix); (tmp_path / "sort_kernels.inc").write_text(sort)
    exe = tmp_path / "sort_host_emulation"
    subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", f"-I{ROOT}/include", f'-DIX_KERNELS_INC="{tmp_path / "ix_kernels.inc"}"', f'-DSORT_KERNELS_INC="{tmp_path / "sort_kernels.inc"}"',
                    os.path.join(ROOT, "tests", "cpp", "sort_host_emulation.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "cases: the kernels' text equals the definition" in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[0]) == 14, r.stdout
