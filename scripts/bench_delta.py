#!/usr/bin/env python3
"""What a device delta costs, measured (profiles/delta/README.md).  No threshold: nobody has measured this before.

The stress_test world (Transform, Velocity, Ttl: 60 B per entity, 14 words) plus Team {1 x u32}, a component no system writes, at `--entities` slots (default
1 M), everyone alive.  Four deltas of frame 1 against frame 0, each fetching Transform.translation (3 x f32) with slots, each with and without
GGRS_DELTA_TRUST_VERSIONS:

  everything   CHANGED, changed = Transform, Velocity, Ttl; one AdvanceFrame between the Saves: every entity moved
  nothing      CHANGED, changed = Team; the same frames: zero rows
  edited 3 %   CHANGED, changed = Transform, Velocity, Ttl; between the Saves one scatter wrote Transform.translation.x of about 3 % of the entities
  despawned    DESPAWNED; between the Saves one scatter despawned every 32nd entity

Each configuration: `--warmup` calls, then `--calls` calls of ggrs_hip_delta_frames through the C ABI, each between two HIP events on the world's stream (first
launch to the count's copy back); the three launches by themselves from the events the library puts around them (ggrs_dbg_query_launch_us: a delta's match, scan
and emit are timed as a query's).  Two yardsticks that are not the code under test, on the same device in the same run:

  (a) copy    a hipMemcpyAsync device-to-device that moves as many bytes as the call reads plus writes -- the mask words of both sides, the compared columns of
              both sides as far as the match launch has to read them (`cmp`: bytes per slot and side, stated per configuration below), the fetched words of
              the rows, the rows written -- as a copy of half that sum, which reads it once and writes it once
  (b) today   the route through the calls that existed before: two World.query calls (every compared word, with slots), their results copied to the host, a
              numpy compare by slot (host clock: it ends in stream waits)

The delta's slots are compared with (b)'s: a mismatch is the only thing that makes this script fail.

    python scripts/bench_delta.py --readme profiles/delta/README.md
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(stream, fn, warmup, calls):
    import torch
    for _ in range(warmup): fn()
    us = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream); fn(); b.record(stream); b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--today-calls", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--readme", default="", help="append the series as a section of this file")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    import torch
    import bevy_ggrs_amd as bg
    import common as cm
    from bevy_ggrs_amd import _ffi
    n = args.entities
    S, A = bg.SaveGameState, bg.AdvanceFrame
    hip = C.CDLL(None)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]; hip.hipMemcpyAsync.restype = C.c_int
    res = {"entities": n, "configs": {}}
    ok = True

    def world():
        stream = torch.cuda.Stream()
        w = bg.World(n, max_depth=3, stream=stream.cuda_stream)
        ids = cm.build_particles(w)
        team = w.register_component("Team", 4, 1)
        T, V, Lc = ids[:3]
        vel, ttl = cm.synthetic_particles(n)
        tcols = [np.full(n, cm.f32bits(cm.TRANSFORM_DEFAULT)[k], dtype=np.uint32) for k in range(10)]
        w.spawn(n, {T: tcols, V: [cm.f32bits(vel[:, 0]), cm.f32bits(vel[:, 1]), np.zeros(n, dtype=np.uint32)], Lc: [ttl], team: [(np.arange(n) % 4).astype(np.uint32)]})
        w.set_depth(3)
        return w, stream, (T, V, Lc, team)

    def between(kind):
        """The world with frames 0 and 1 saved and `kind` between them."""
        w, stream, ids = world()
        T = ids[0]
        w.handle_requests([S(0)])
        if kind == "advance": w.handle_requests([A((0,)), S(1)])
        else:
            if kind == "edit":
                slots = np.flatnonzero(np.random.default_rng(11).random(n) < 0.03).astype(np.uint32)
                w.scatter(slots, {(T, 0): np.full(slots.size, np.float32(123.5).view(np.uint32), dtype=np.uint32)}, op="write")
            else: w.scatter(np.arange(0, n, 32, dtype=np.uint32), op="despawn")
            w.set_frame(1); w.handle_requests([S(1)])
        return w, stream, ids

    # name -> (what lies between the Saves, kind, changed, cmp: compared bytes per slot and side the match launch has to read, without and with TRUST_VERSIONS)
    #   everything: every lane matches on Transform's first DIFF_BATCH = 4 columns, nothing more is read; nothing: Team's one word, or with the versions trusted
    #   no column at all; edited: no unit is decided early, all 14 words (60 B), or with the versions trusted Transform's ten (the scatter wrote one of its columns)
    cases = {"everything": ("advance", "changed", (0, 1, 2), (16, 16)), "nothing": ("advance", "changed", (3,), (4, 0)),
             "edited 3 %": ("edit", "changed", (0, 1, 2), (60, 40)), "despawned": ("despawn", "despawned", (), (0, 0))}
    worlds = {}
    for name, (how, kind, changed, cmp_bytes) in cases.items():
        if how not in worlds:
            for old in worlds.values(): old[0].close()
            worlds.clear(); worlds[how] = between(how)
        w, stream, ids = worlds[how]
        T = ids[0]
        lib, p = w._lib, w._p
        fetch = [(T, 0), (T, 1), (T, 2)]
        comps = [ids[c] for c in changed]
        for trust in (False, True):
            desc = w.delta_desc(fetch, kind=kind, changed=comps, trust_versions=trust)
            lay = w.query_layout(desc.q, n)
            out = torch.empty(int(lay.total_bytes), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rep = _ffi.DeltaReport()

            def call(): assert lib.ggrs_hip_delta_frames(p, 1, 0, C.byref(desc), out.data_ptr(), n, C.byref(rep)) == 0
            call()
            r = timed(stream, call, args.warmup, args.calls)
            assert lib.ggrs_dbg_query_launch_us(p, 1, None) == 0
            per = []
            for _ in range(args.calls):
                call()
                us = (C.c_double * 3)(); lib.ggrs_dbg_query_launch_us(p, 1, us); per.append(list(us))
            lib.ggrs_dbg_query_launch_us(p, 0, None)
            r["match_us"], r["scan_us"], r["emit_us"] = (round(statistics.median(x[k] for x in per), 2) for k in range(3))
            matched = int(rep.n_matched)
            units = (n + 63) // 64
            n_masks = 2 + 1 + 2 * len(comps)                                       # alive of both sides, Transform's presence (the fetch), presence of both sides per asked component
            cmpb = cmp_bytes[1 if trust else 0]
            read = n_masks * units * 8 + 2 * cmpb * n + units * 8 * 2 + matched * 12   # ... the match and scan words read again by scan and emit, the fetched words
            written = units * 8 * 2 + matched * (12 + 4)
            r.update(n_matched=matched, cmp_bytes_per_slot_and_side=cmpb, bytes_read=read, bytes_written=written)
            half = (read + written) // 2
            src, dst = torch.zeros(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def copy(): assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), half, 3, stream.cuda_stream) == 0      # 3: hipMemcpyDeviceToDevice
            r["copy_us"] = timed(stream, copy, args.warmup, args.calls)["median_us"]
            del src, dst
            # (b) today's route, and the check: the same slots
            words = [(c, k) for c in comps for k in range(w._comps[c][2])]
            host_us = []
            for _ in range(args.today_calls):
                t0 = time.perf_counter()
                if kind == "despawned":
                    s_new, s_old = w.query(1, [], max_rows=n).numpy()[0], w.query(0, [], max_rows=n).numpy()[0]
                    rows = np.setdiff1d(s_old, s_new, assume_unique=True)
                else:
                    # (every entity of this world has every component on both sides: the rows are the slots of new that old lacks or holds other words for)
                    s_new, c_new = w.query(1, words, max_rows=n).numpy()
                    s_old, c_old = w.query(0, words, max_rows=n).numpy()
                    _, i_new, i_old = np.intersect1d(s_new, s_old, assume_unique=True, return_indices=True)
                    differs = np.zeros(i_new.size, dtype=bool)
                    for a, b in zip(c_new, c_old): differs |= a[i_new] != b[i_old]
                    rows = np.union1d(s_new[i_new][differs], np.setdiff1d(s_new, s_old, assume_unique=True))
                host_us.append((time.perf_counter() - t0) * 1e6)
            r["today_us"] = round(statistics.median(host_us), 1)
            got = w.delta(1, 0, fetch, kind=kind, changed=comps, trust_versions=trust, out=out, max_rows=n)
            same = got.n_matched == matched == rows.size and np.array_equal(got.numpy()[0], rows.astype(np.uint32))
            ok = ok and same
            r["matches_todays_route"] = bool(same)
            r["over_copy"] = round(r["median_us"] / r["copy_us"], 2)
            r["today_over_delta"] = round(r["today_us"] / r["median_us"], 1)
            res["configs"][f"{name}{', versions trusted' if trust else ''}"] = r
            del out
    for old in worlds.values(): old[0].close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(res, indent=1) + "\n")
    if args.readme:
        lines = ["", f"### Measured: {n} slots of the stress_test world, frame 1 against frame 0, {args.calls} calls after {args.warmup}", "",
                 "| configuration | rows | cmp B per slot and side | bytes read + written | median us per call (min .. max) | match / scan / emit launch us | (a) copy of the same bytes us | call / (a) | (b) today's route us | (b) / call |",
                 "|---|---|---|---|---|---|---|---|---|---|"]
        for k, r in res["configs"].items():
            lines.append(f"| {k} | {r['n_matched']} | {r['cmp_bytes_per_slot_and_side']} | {r['bytes_read']} + {r['bytes_written']} | {r['median_us']} ({r['min_us']} .. {r['max_us']}) | "
                         f"{r['match_us']} / {r['scan_us']} / {r['emit_us']} | {r['copy_us']} | {r['over_copy']} | {r['today_us']} | {r['today_over_delta']} |")
        with open(args.readme, "a") as f: f.write("\n".join(lines) + "\n")
    if not ok:
        print("MISMATCH: a delta's slots differ from what two queries and a host compare give", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
