"""Remote inserts that carry the sender's value (ggrs_hip_add_custom_system_values): e.val_*(j, k) / e.send_value(slot, j) -- the sender's staged words go to a payload
array at its own slot, the key (g + 1) << 40 | (slot + 1) into the target's winner word with one 64-bit atomic max, and k_apply_remote gathers the winner's words.
Everything goes through the C ABI and is bit-exact: the Checksum(u128) of every SaveGameState, the final state (alive, every presence mask ANDed with alive and cut
at len, every word of every present component) and every frame the ring holds equal the CPU oracle's, whose apply callback mirrors the conflict rules
(remote_values_common.py).  The oracle sessions are computed once per scenario and shared, unchanged; the two "floor" sessions are the ones
test_remote_values_text.py holds to the coverage floors.

Shapes: 1 slot (one lane), 64 (one full wave), 65 (a wave boundary), 257 (several workgroups of the apply), 1025 (one past a 1024-slot workgroup tile of the tick
kernel), 8262 (one past an 8192-slot layout tile: gathers and sends cross layout tiles; 9 ticks -- the oracle calls Python once per entity, system and frame)."""
import ctypes as C
import os

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
from bevy_ggrs_amd import _ffi
from remote_values_common import build_brand, spawn_brand, strike_links
from test_remote_values_text import DEPTH, SCENARIOS, oracle_session, scenario_lists      # (names only: the scenarios and their cached oracle sessions)

pytestmark = pytest.mark.gpu


def _ring_states(w, ids):
    """Every frame the ring holds, loaded newest first (a Load pops the newer snapshots) and snapshotted."""
    out = {}
    for f in reversed([f for f in range(w.frame + 1) if w.has_snapshot(f)]):
        w.load(f)
        out[f] = cm.snapshot_state(w, ids)
    return out


_REF_RINGS = {}


def _reference(name):
    """(checksums, final state, {frame: state} of the oracle's ring) of a scenario; the ring is walked once (it rewinds the oracle world) and kept."""
    cks, final, o, ids, st = oracle_session(name)
    if name not in _REF_RINGS: _REF_RINGS[name] = _ring_states(o, ids)
    return cks, final, _REF_RINGS[name]


def _gpu_world(name, before=None, values=True):
    n, cd, ticks, kw, links = SCENARIOS[name]
    g = bg.World(n + 128, max_depth=DEPTH)
    if before: before(g)
    ids = build_brand(g, n, values=values, **kw); spawn_brand(g, ids, n, links=None if links is None else links(n)); g.set_depth(DEPTH)
    g.set_synctest_check_distance(cd)
    return g, ids


def _gpu_session(name, before=None):
    g, ids = _gpu_world(name, before)
    lists = scenario_lists(name)
    cks = []
    for k, reqs in enumerate(lists):
        cks += g.handle_requests(reqs)
        # the invariant, after EVERY list: the remote inbox and both components' winner words are all zeros whenever a host call returns
        assert not _inbox(g).any() and not _winners(g, ids[3]).any() and not _winners(g, ids[4]).any(), f"{name}: something is left in the inbox or the winner words after list {k}"
    frames = [r.frame for reqs in lists for r in reqs if isinstance(r, bg.SaveGameState)]
    return g, ids, list(zip(frames, cks)), lists


def _compare(g, ids, cks, ref, ctx):
    want, final, ring_states = ref
    assert len(cks) == len(want) > 0, (len(cks), len(want))
    for (fa, ca), (fb, cb) in zip(cks, want):
        assert fa == fb and ca == cb, f"{ctx}: frame {fa}: gpu {ca:#x} oracle {cb:#x}"
    cm.assert_states_equal(cm.snapshot_state(g, ids), final, ctx)
    got = _ring_states(g, ids)
    assert sorted(got) == sorted(ring_states) and len(got) >= 2, (sorted(got), sorted(ring_states))
    for f in got: cm.assert_states_equal(got[f], ring_states[f], f"{ctx}: ring frame {f}")
    return got


def _inbox(g):
    """The remote inbox as the device holds it once everything queued has run (ggrs_dbg_remote_inbox)."""
    g._lib.ggrs_dbg_remote_inbox.restype = C.c_int64
    g._lib.ggrs_dbg_remote_inbox.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    buf = np.full(1 << 16, 0xA5A5A5A5, dtype=np.uint32)
    n = g._lib.ggrs_dbg_remote_inbox(g._p, buf.ctypes.data, buf.nbytes)
    assert 0 < n <= buf.nbytes and n % 4 == 0, n
    return buf[:n // 4]


def _winners(g, comp):
    """The winner words of a value-bound component as the device holds them once everything queued has run (ggrs_dbg_value_winners)."""
    g._lib.ggrs_dbg_value_winners.restype = C.c_int64
    g._lib.ggrs_dbg_value_winners.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
    buf = np.full(1 << 15, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    n = g._lib.ggrs_dbg_value_winners(g._p, comp, buf.ctypes.data, buf.nbytes)
    assert 0 < n <= buf.nbytes and n % 8 == 0, n
    return buf[:n // 8]


def _applies(g):
    info = g.kernel_info()
    return int(info["remote_inbox"].split("(")[-1].split(" applies")[0]), info


def _is_value_world(g, ids, lists):
    n_adv = sum(isinstance(r, bg.AdvanceFrame) for reqs in lists for r in reqs)
    applies, info = _applies(g)
    assert info["request_group_kernel"].startswith("ggrs_jit_tick"), info
    assert info["group_caps"].endswith("/ 1 steps") and info["remote_inbox"].startswith("one u32 per slot, 2 remotely commanded components"), info
    assert info["value_inbox"].startswith("2 value-bound components") and "4 value bindings" in info["value_inbox"] and f"({n_adv} applies so far)" in info["value_inbox"], info
    assert int(info["value_inbox"].split(" bytes allocated")[0].split(" ")[-1]) > 0, info
    assert info["lazy_live_block"].startswith("off") and info["deferred_saves"].startswith("off"), info
    assert applies == n_adv > 0, (applies, n_adv)                            # one apply per AdvanceWorld executed
    # the invariants: the inbox and both components' winner words are all zeros whenever no group-and-apply pair is in flight
    assert not _inbox(g).any() and not _winners(g, ids[3]).any() and not _winners(g, ids[4]).any()
    assert g._lib.ggrs_dbg_value_winners(g._p, ids[0], None, 0) == -1        # Hp: no value binding names it


@pytest.mark.parametrize("name", ["1", "64", "65", "257", "1025", "8262"])
def test_brand_synctest_at_check_distance_7_against_the_oracle(name):
    """Every Save's checksum, the final live state and every frame the ring holds."""
    ref = _reference(name)
    g, ids, cks, lists = _gpu_session(name)
    _is_value_world(g, ids, lists)
    _compare(g, ids, cks, ref, f"brand {name}")
    n, final = SCENARIOS[name][0], ref[1]
    B, M = ids[3], ids[4]
    if n >= 64:
        pb = final[f"present{B}"]
        assert pb.any() and final[f"present{M}"].any()
        src = final[f"c{B}w2"][pb]
        assert (src != 0xFFFFFFFF).any() and (src[src != 0xFFFFFFFF] < n).all()                     # values landed: the source is a sender's slot, not the default
    if n > 8192:
        links, i = strike_links(n), np.arange(n)
        assert ((links < n) & ((links >> np.uint64(13)) != (i >> 13).astype(np.uint64))).any()      # a sender in one 8192-slot layout tile, its target in the other
        pb = final[f"present{B}"]; src = final[f"c{B}w2"]
        far = pb & (src != 0xFFFFFFFF) & ((src >> 13) != (i >> 13))
        assert far.any() and pb[8192:].any() and pb[:8192].any()                                    # ... and such a value arrived: a gather across layout tiles


def test_every_entity_targets_slot_0_the_highest_key_wins_and_its_three_words_arrive_together():
    name = "8262 all to 0"
    ref = _reference(name)
    g, ids, cks, lists = _gpu_session(name)
    _is_value_world(g, ids, lists)
    ring = _compare(g, ids, cks, ref, "all to slot 0")
    n = SCENARIOS[name][0]
    H, T, P, B, M = ids
    # In every frame some tagger (the highest ordinal on Burn) sends to slot 0, so the frame's winner is the tagger at the HIGHEST live slot with (slot + frame) % 6 == 0.
    # Ring frame f holds the world as the step that saw f.frame == f left it: slot 0 burns with ticks 9 (the tagger's; not yet counted down), `source` is that sender's slot -- near the
    # top of the world, of the right residue --, and dps is THAT sender's power * 2: the three words arrive together, no mixture of two senders' words passes
    power = (3 + (np.arange(n) * 7) % 29).astype(np.float32)
    seen = 0
    for f, stt in ring.items():
        if f == 0: continue
        assert stt["alive"][0] and stt[f"present{B}"][0], f
        dps = np.array([stt[f"c{B}w0"][0]], dtype=np.uint32).view(np.float32)[0]; ticks = int(stt[f"c{B}w1"][0]); src = int(stt[f"c{B}w2"][0])
        assert ticks == 9 and n - 64 <= src < n and (src + f) % 6 == 0, (f, ticks, src)
        assert dps == power[src] * np.float32(2.0), (f, src, dps, power[src])
        assert int(stt[f"c{M}w0"][0]) & 0xFFFFFFFF >= n - 64 and int(stt[f"c{M}w0"][0]) >> 32 == int(power[int(stt[f"c{M}w0"][0]) & 0xFFFFFFFF]), f      # Mark: the halves of one u64 from one sender
        seen += 1
    assert seen >= 7


def test_p2p_shaped_lists_with_rollbacks_of_0_to_7_frames_and_host_decided_spawns():
    """The spawn variant: a child cannot be hit in the frame it appears (the oracle session counted such sends)."""
    ref = _reference("floor p2p")
    g, ids, cks, lists = _gpu_session("floor p2p")
    depths = sorted({sum(isinstance(r, bg.AdvanceFrame) for r in reqs) - 1 for reqs in lists[1:]})
    assert depths == list(range(8)), depths
    _is_value_world(g, ids, lists)
    _compare(g, ids, cks, ref, "brand p2p")
    assert oracle_session("floor p2p")[4].spawned_this_frame >= 3 and ref[1]["len"] >= 300 + 10


def test_host_decided_spawns_under_synctest():
    ref = _reference("floor synctest")
    g, ids, cks, lists = _gpu_session("floor synctest")
    _is_value_world(g, ids, lists)
    _compare(g, ids, cks, ref, "brand with spawns")
    assert ref[1]["len"] >= 300 + 10 and oracle_session("floor synctest")[4].spawned_this_frame >= 3


def test_the_effect_variant_takes_the_fused_apply():
    ref = _reference("effects")
    g, ids, cks, lists = _gpu_session("effects")
    _is_value_world(g, ids, lists)
    info = g.kernel_info()
    n_adv = sum(isinstance(r, bg.AdvanceFrame) for reqs in lists for r in reqs)
    assert "effect_inbox" in info and f"({n_adv} applies so far)" in info["effect_inbox"], info
    _compare(g, ids, cks, ref, "brand with effects")


def _raw_ring(g, ids):
    """Every frame the ring holds, newest first: the masks and EVERY word of every column below len as the block holds them -- dead and absent slots too."""
    out = {}
    for f in reversed([f for f in range(g.frame + 1) if g.has_snapshot(f)]):
        g.load(f)
        n = g.len
        rec = [g.alive_mask(n).tobytes()]
        for c in ids:
            rec.append(g.present_mask(c, n).tobytes())
            for k in range(g._comps[c][2]): rec.append(g.download_word(c, k, 0, n).tobytes())
        out[f] = b"".join(rec)
    return out


def test_specialised_copies_forced_and_the_generic_kernel_forced_give_the_same_bytes(monkeypatch):
    ref = _reference("257")
    runs = {}
    for how in ("specialised", "generic"):
        if how == "specialised":
            monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1"); monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
            g, ids, cks, lists = _gpu_session("257", before=lambda w: w._lib.ggrs_dbg_set_spec_shapes(w._p, 3))
            assert g.kernel_info()["specialised_kernel"].startswith("ready"), g.kernel_info()["specialised_kernel"]
        else:
            monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1000000"); monkeypatch.delenv("GGRS_JIT_SPECIALISE_SYNC", raising=False)
            g, ids, cks, lists = _gpu_session("257")
            assert not g.kernel_info()["specialised_kernel"].startswith("ready"), g.kernel_info()["specialised_kernel"]
        _is_value_world(g, ids, lists)
        raw = _raw_ring(g, ids)
        g, ids, cks2, lists = _gpu_session("257", before=(lambda w: w._lib.ggrs_dbg_set_spec_shapes(w._p, 3)) if how == "specialised" else None)
        assert cks2 == cks
        _compare(g, ids, cks, ref, f"{how} kernel")
        runs[how] = (cks, raw)
    assert runs["specialised"][0] == runs["generic"][0] and sorted(runs["specialised"][1]) == sorted(runs["generic"][1]) and len(runs["generic"][1]) >= 7
    for f in runs["generic"][1]: assert runs["specialised"][1][f] == runs["generic"][1][f], f"ring frame {f}"


def test_no_launch_more_than_the_same_world_with_send_insert_only():
    """[Save(f), Advance] lists, one frame each: the value world's frame is the group's launch plus ONE apply -- exactly the launches of the same world whose torch
    and tagger use send_insert of the default."""
    counts = {}
    frames = 6
    for values in (True, False):
        g, ids = _gpu_world("257", values=values)
        g.set_synctest_check_distance(-1)
        g.handle_requests([bg.SaveGameState(0), bg.AdvanceFrame((1,))])          # (the first list: whatever a first launch does besides)
        g.host_timeline(1)
        for f in range(1, 1 + frames): g.handle_requests([bg.SaveGameState(f), bg.AdvanceFrame((f % 3,))])
        counts[values] = g.host_timeline(0)["launches"]
        assert _applies(g)[0] == frames + 1 and not _inbox(g).any()
        if values: assert not _winners(g, ids[3]).any() and not _winners(g, ids[4]).any()
    assert counts[True] == counts[False] >= 2 * frames, counts


def _fanout_rank(rank, size, id_q, q):
    """ggrs_hip_fanout_step's request-list form on the brand world at world size 1."""
    try:
        from bevy_ggrs_amd.fanout import RcclFanout
        n = 257
        g = bg.World(n + 128, max_depth=6, device=0)
        ids = build_brand(g, n); spawn_brand(g, ids, n); g.set_depth(6)
        native = RcclFanout(g, rank, size, RcclFanout.unique_id())
        reqs = [bg.SaveGameState(0)]
        for b in range(2):
            reqs += [bg.LoadGameState(0), bg.AdvanceFrame((b + 1,)), bg.SaveGameState(1), bg.AdvanceFrame((b + 1,)), bg.SaveGameState(2)]
        ns = native.step(reqs)
        table = native.collect()
        got = [int(p[0]) | (int(p[1]) << 64) for p in np.asarray(table).reshape(-1, 2)]
        clean = not _inbox(g).any() and not _winners(g, ids[3]).any() and not _winners(g, ids[4]).any()
        # ... and branch steps are refused with a message
        pre, keep, _ = g.build_requests([bg.SaveGameState(2)])
        inputs = np.zeros((2, 2, 1), dtype=np.uint8)
        bs = _ffi.BranchStep()
        bs.prefix, bs.n_prefix, bs.n_branches, bs.n_frames, bs.n_inputs, bs.flags = pre, 1, 2, 2, 1, _ffi.BRANCH_SAVE_LAST
        bs.inputs = inputs.ctypes.data
        rc = _ffi.lib.ggrs_hip_fanout_step_branches(native._p, C.byref(bs), None)
        msg = (_ffi.lib.ggrs_hip_fanout_last_error(native._p) or b"").decode()
        native.close()
        q.put((rank, "ok", ns, got, clean, rc, msg))
    except Exception as e:                                    # noqa: BLE001
        import traceback
        q.put((rank, "error", f"{type(e).__name__}: {e}", traceback.format_exc()))


def test_fanout_step_works_at_world_size_1_and_branch_steps_are_refused_with_a_message():
    import multiprocessing as mp
    from oracle.binding import FLAT, OracleWorld
    from test_gpu_zfanout import _double_lib                                                   # (a name only: no test is imported)
    ctx = mp.get_context("spawn")
    q, id_q = ctx.Queue(), ctx.Queue()
    old = os.environ.get("GGRS_RCCL_LIB")
    os.environ["GGRS_RCCL_LIB"] = _double_lib()
    try:
        p = ctx.Process(target=_fanout_rank, args=(0, 1, id_q, q)); p.start()
    finally:
        if old is None: os.environ.pop("GGRS_RCCL_LIB", None)
        else: os.environ["GGRS_RCCL_LIB"] = old
    try: r = q.get(timeout=240)
    finally:
        p.join(timeout=60)
        if p.is_alive(): p.kill()
    assert r[1] == "ok" and r[2] == 5 and r[4], r
    # the oracle's walk of the same list
    n = 257
    o = OracleWorld(n + 128, 6, FLAT); ido = build_brand(o, n); spawn_brand(o, ido, n); o.set_depth(6)
    want = []
    reqs = [bg.SaveGameState(0)]
    for b in range(2): reqs += [bg.LoadGameState(0), bg.AdvanceFrame((b + 1,)), bg.SaveGameState(1), bg.AdvanceFrame((b + 1,)), bg.SaveGameState(2)]
    for rq in reqs: want += o.handle_requests([rq])
    assert r[3] == want and len(set(want[1:])) == 4, (r[3], want)           # the checksums are the oracle's; the branches diverge, and so do their frames
    assert r[5] == bg.GGRS_E_INVALID and "value bindings" in r[6] and "ggrs_hip_fanout_step_branches" in r[6] and "use ggrs_hip_fanout_step" in r[6], r
