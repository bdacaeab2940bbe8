#!/usr/bin/env python3
"""What a device query costs, measured (profiles/query/README.md).  No threshold: nobody has measured this before.

The stress_test world (Transform, Velocity, Ttl: 60 B per entity, 14 words) at `--entities` slots (default 1 M), at two densities:

  dense     everyone alive
  sparse    about 3 % alive: the particles steady state, where RollbackOrdered::len has grown 30 x beyond the live entities (97 % of the slots were spawned with a
            Ttl of 1 and the world's own despawn_after_ttl killed them in two AdvanceFrames)

and two queries of the live world, each with slots:

  translation   Transform.translation (3 x f32)
  all           all 14 words

Each configuration: `--warmup` calls, then `--calls` calls of ggrs_hip_query through the C ABI, each between two HIP events on the world's stream (first launch to
the count's copy back); the three launches by themselves from the events the library puts around them (ggrs_dbg_query_launch_us).  Two yardsticks that are not the
code under test, on the same device in the same run:

  (a) copy    a hipMemcpyAsync device-to-device that moves as many bytes as the query reads plus writes: the masks and the fetched words of the matching rows
              read, the rows written -- a copy of half that sum, which reads it once and writes it once
  (b) today   the route through the calls that existed before: download_alive, one download_word per fetched word over [0, len), numpy compaction on the host
              (host clock: it ends in stream waits)

The query's rows are compared with (b)'s, which is the model of tests/query_common.py over the same downloads: a mismatch is the only thing that makes this script
fail.

    python scripts/bench_query.py --readme profiles/query/README.md
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
    import query_common as qc
    from bevy_ggrs_amd import _ffi
    n = args.entities
    hip = C.CDLL(None)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]; hip.hipMemcpyAsync.restype = C.c_int
    res = {"entities": n, "configs": {}}
    ok = True
    for density in ("dense", "sparse"):
        stream = torch.cuda.Stream()
        w = bg.World(n, max_depth=3, stream=stream.cuda_stream)
        ids = cm.build_particles(w)
        T, V, Lc = ids[:3]
        vel, ttl = cm.synthetic_particles(n)
        if density == "sparse":
            ttl = np.where(np.random.default_rng(7).random(n) < 0.033, np.uint64(1 << 40), np.uint64(1)).astype(np.uint64)
        cm.spawn_particles(w, ids, n, vel, ttl)
        w.set_depth(3)
        w.handle_requests([bg.AdvanceFrame((0,)), bg.AdvanceFrame((0,))])
        alive_n = w.active_count()
        lib, p = w._lib, w._p
        queries = {"translation": [(T, 0), (T, 1), (T, 2)], "all": [(T, k) for k in range(10)] + [(V, k) for k in range(3)] + [(Lc, 0)]}
        for qname, fetch in queries.items():
            desc = w.query_desc(fetch, slots=True)
            lay = w.query_layout(desc, n)
            out = torch.empty(int(lay.total_bytes), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rep = _ffi.QueryReport()

            def call(): assert lib.ggrs_hip_query(p, bg.LIVE, C.byref(desc), out.data_ptr(), n, C.byref(rep)) == 0
            call()
            r = timed(stream, call, args.warmup, args.calls)
            # the launches by themselves: the library's own events around match, scan and emit
            assert lib.ggrs_dbg_query_launch_us(p, 1, None) == 0
            per = []
            for _ in range(args.calls):
                call()
                us = (C.c_double * 3)(); lib.ggrs_dbg_query_launch_us(p, 1, us); per.append(list(us))
            lib.ggrs_dbg_query_launch_us(p, 0, None)
            r["match_us"], r["scan_us"], r["emit_us"] = (round(statistics.median(x[k] for x in per), 2) for k in range(3))
            matched = int(rep.n_matched)
            wbs = [w._comps[c][1] for c, _ in fetch]
            n_masks = 1 + len({c for c, _ in fetch})
            read = n_masks * ((n + 63) // 64) * 8 + matched * sum(wbs)
            written = matched * (sum(wbs) + 4)
            r.update(alive=alive_n, n_matched=matched, words=len(fetch), bytes_read=read, bytes_written=written)
            # (a) a device-to-device copy that moves the same bytes
            half = (read + written) // 2
            src, dst = torch.zeros(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def copy(): assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), half, 3, stream.cuda_stream) == 0      # 3: hipMemcpyDeviceToDevice
            r["copy_us"] = timed(stream, copy, args.warmup, args.calls)["median_us"]
            del src, dst
            # (b) today's route, and the check: the same rows
            host_us = []
            for _ in range(args.today_calls):
                t0 = time.perf_counter()
                alive = w.alive_mask(n)
                cols = [w.download_word(c, k, 0, n) for c, k in fetch]
                rows = np.flatnonzero(alive)
                packed = [col[rows] for col in cols]
                host_us.append((time.perf_counter() - t0) * 1e6)
            r["today_us"] = round(statistics.median(host_us), 1)
            slots, got = w.query(bg.LIVE, fetch, out=out, max_rows=n).numpy()
            rec = {"len": n, "alive": alive, "present": {c: w.present_mask(c, n) for c in {c for c, _ in fetch}}, "columns": dict(zip(fetch, cols))}
            want = qc.model_of(rec, qc.make_desc(fetch), n)
            same = matched == want["n_matched"] and np.array_equal(slots, want["slots"]) and all(np.array_equal(a, b) for a, b in zip(got, want["columns"]))
            same = same and all(np.array_equal(a, b) for a, b in zip(packed, want["columns"]))
            ok = ok and same
            r["matches_model"] = bool(same)
            r["over_copy"] = round(r["median_us"] / r["copy_us"], 2); r["emit_over_copy"] = round(r["emit_us"] / r["copy_us"], 2)
            r["today_over_query"] = round(r["today_us"] / r["median_us"], 1)
            r["emit_gb_per_s"] = round((matched * sum(wbs) + written) / max(r["emit_us"], 1e-9) / 1e3, 1)
            res["configs"][f"{density}, {qname}"] = r
            del out
        w.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(res, indent=1) + "\n")
    if args.readme:
        lines = ["", f"### Measured: {n} slots of the stress_test world, the live world, {args.calls} calls after {args.warmup}", "",
                 "| configuration | alive | rows | bytes read + written | median us per call (min .. max) | match / scan / emit launch us | (a) copy of the same bytes us | call / (a) | emit / (a) | emit GB/s | (b) today's route us | (b) / call |",
                 "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for k, r in res["configs"].items():
            lines.append(f"| {k} | {r['alive']} | {r['n_matched']} | {r['bytes_read']} + {r['bytes_written']} | {r['median_us']} ({r['min_us']} .. {r['max_us']}) | {r['match_us']} / {r['scan_us']} / {r['emit_us']} | "
                         f"{r['copy_us']} | {r['over_copy']} | {r['emit_over_copy']} | {r['emit_gb_per_s']} | {r['today_us']} | {r['today_over_query']} |")
        with open(args.readme, "a") as f: f.write("\n".join(lines) + "\n")
    if not ok:
        print("MISMATCH: a query's rows differ from the model over the downloaded state", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
