#!/usr/bin/env python3
"""What ordering a query's rows on the device costs, measured (profiles/sorted_query/README.md).  No threshold: nobody has measured this before.

The stress_test world (Transform, Velocity, Ttl: 60 B per entity, 14 words) at 10 k, 100 k and 1 M slots, everyone alive, the live world.  The rows are
Transform.translation (3 x f32) with slots, in two orders:

  f32          Transform.translation.x ascending (GGRS_SORT_F): one stage, four radix passes
  ttl+f32      the u64 Ttl descending, then translation.x: three stages, twelve passes, two rekey gathers

Each configuration: `--warmup` calls, then `--calls` calls of ggrs_hip_query_sorted through the C ABI, each between two HIP events on the world's stream; the
phases by themselves -- match, scan, the host's read of the count plus the rows launch, the stages, the emit -- from the events the library puts around
them (ggrs_dbg_sorted_query_launch_us).  Two references that are not the code under test, in the same run:

  (a) query   ggrs_hip_query of the same desc: what the order costs on top of the gather; its emit launch by itself is what the sorted emit, whose loads are a
              gather, is set against (bytes moved per second)
  (b) today   the query's rows copied to the host and np.lexsort over the transformed keys and the slot (host clock: it ends in a stream wait)

and the small form against the large form on results of 512, 1024 and 2048 rows (ggrs_dbg_set_sort_form): the stages' time, one launch against twelve.
The sorted rows are compared with (b)'s order: a mismatch is the only thing that makes this script fail.

    python scripts/bench_sorted_query.py --readme profiles/sorted_query/README.md
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
    ap.add_argument("--entities", type=int, nargs="*", default=[10_000, 100_000, 1_000_000])
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
    import sorted_query_common as sq
    from bevy_ggrs_amd import _ffi
    res = {"configs": {}, "forms": {}}
    ok = True

    def world(n, stream):
        w = bg.World(n, max_depth=3, stream=stream.cuda_stream)
        ids = cm.build_particles(w)
        vel, ttl = cm.synthetic_particles(n)
        cm.spawn_particles(w, ids, n, vel, ttl)
        w.set_depth(3)
        w.handle_requests([bg.AdvanceFrame((0,)), bg.AdvanceFrame((0,))])
        return w, ids[:3]

    def phases(lib, p, call, calls):
        assert lib.ggrs_dbg_sorted_query_launch_us(p, 1, None) == 0
        per = []
        for _ in range(calls):
            call()
            us = (C.c_double * 5)(); lib.ggrs_dbg_sorted_query_launch_us(p, 1, us); per.append(list(us))
        lib.ggrs_dbg_sorted_query_launch_us(p, 0, None)
        return [round(statistics.median(x[k] for x in per), 2) for k in range(5)]

    for n in args.entities:
        stream = torch.cuda.Stream()
        w, (T, V, Lc) = world(n, stream)
        lib, p = w._lib, w._p
        fetch = [(T, 0), (T, 1), (T, 2)]
        desc = w.query_desc(fetch, slots=True)
        lay = w.query_layout(desc, n)
        out = torch.empty(int(lay.total_bytes), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rep = _ffi.QueryReport()
        # (a) the query of the same desc, and its emit launch by itself
        def query(): assert lib.ggrs_hip_query(p, bg.LIVE, C.byref(desc), out.data_ptr(), n, C.byref(rep)) == 0
        query()
        q = timed(stream, query, args.warmup, args.calls)
        assert lib.ggrs_dbg_query_launch_us(p, 1, None) == 0
        per = []
        for _ in range(args.calls):
            query()
            us = (C.c_double * 3)(); lib.ggrs_dbg_query_launch_us(p, 1, us); per.append(list(us))
        lib.ggrs_dbg_query_launch_us(p, 0, None)
        q_emit_us = round(statistics.median(x[2] for x in per), 2)
        moved = int(rep.n_matched) * (12 + 12 + 4)                                   # the emit's bytes: the fetched words read, the rows and the slots written
        x_col, ttl_col = w.download_word(T, 0, 0, n), w.download_word(Lc, 0, 0, n)
        for oname, order_by in (("f32", [(T, 0, "f")]), ("ttl+f32", [(Lc, 0, "u", "desc"), (T, 0, "f")])):
            sdesc = w.sort_desc(order_by)

            def call(): assert lib.ggrs_hip_query_sorted(p, bg.LIVE, C.byref(desc), C.byref(sdesc), out.data_ptr(), n, C.byref(rep)) == 0
            call()
            r = timed(stream, call, args.warmup, args.calls)
            r["match_us"], r["scan_us"], r["rows_us"], r["stages_us"], r["emit_us"] = phases(lib, p, call, args.calls)
            matched = int(rep.n_matched)
            r.update(n_matched=matched, query_us=q["median_us"], over_query=round(r["median_us"] / q["median_us"], 2), query_emit_us=q_emit_us)
            r["emit_gb_per_s"] = round((moved + matched * 4) / max(r["emit_us"], 1e-9) / 1e3, 1)        # (+ the permutation read)
            r["query_emit_gb_per_s"] = round(moved / max(q_emit_us, 1e-9) / 1e3, 1)
            # (b) today's route: the query's rows on the host, np.lexsort
            host_us, order = [], None
            for _ in range(args.today_calls):
                t0 = time.perf_counter()
                slots, cols = w.query(bg.LIVE, fetch, out=out, max_rows=n).numpy()
                images = [sq.key_image((x_col if (c, k) == (T, 0) else ttl_col)[slots], 4 if c == T else 8, kind, len(rest) == 1) for c, k, kind, *rest in order_by]
                order = np.lexsort([slots] + images[::-1])
                sorted_cols = [col[order] for col in cols]
                host_us.append((time.perf_counter() - t0) * 1e6)
            r["today_us"] = round(statistics.median(host_us), 1); r["today_over_call"] = round(r["today_us"] / r["median_us"], 1)
            got_slots, got_cols = w.query_sorted(bg.LIVE, fetch, order_by, out=out, max_rows=n).numpy()
            same = np.array_equal(got_slots, slots[order]) and all(np.array_equal(a, b) for a, b in zip(got_cols, sorted_cols))
            ok = ok and same
            r["matches_host_sort"] = bool(same)
            res["configs"][f"{n}, {oname}"] = r
        del out
        w.close()
    # the small form against the large form near IX_TILE rows
    stream = torch.cuda.Stream()
    for n in (512, 1024, 2048):
        w, (T, V, Lc) = world(n, stream)
        lib, p = w._lib, w._p
        desc, sdesc = w.query_desc([(T, 0), (T, 1), (T, 2)], slots=True), w.sort_desc([(T, 0, "f")])
        out = torch.empty(int(w.query_layout(desc, n).total_bytes), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rep = _ffi.QueryReport()

        def call(): assert lib.ggrs_hip_query_sorted(p, bg.LIVE, C.byref(desc), C.byref(sdesc), out.data_ptr(), n, C.byref(rep)) == 0
        row = {}
        for form, name in ((0, "small"), (1, "large")):
            assert lib.ggrs_dbg_set_sort_form(p, form) == 0
            call()
            row[name + "_call_us"] = timed(stream, call, args.warmup, args.calls)["median_us"]
            row[name + "_stages_us"] = phases(lib, p, call, args.calls)[3]
        lib.ggrs_dbg_set_sort_form(p, 0)
        res["forms"][str(n)] = row
        w.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(res, indent=1) + "\n")
    if args.readme:
        lines = ["", f"### Measured: the stress_test world, everyone alive, the live world, translation (3 x f32) + slots, {args.calls} calls after {args.warmup}", "",
                 "| slots, order | rows | median us per call (min .. max) | match / scan / count read + rows / stages / emit us | (a) query of the same desc us | call / (a) | emit GB/s (the query's emit) | (b) host copy + np.lexsort us | (b) / call |",
                 "|---|---|---|---|---|---|---|---|---|"]
        for k, r in res["configs"].items():
            lines.append(f"| {k} | {r['n_matched']} | {r['median_us']} ({r['min_us']} .. {r['max_us']}) | {r['match_us']} / {r['scan_us']} / {r['rows_us']} / {r['stages_us']} / {r['emit_us']} | {r['query_us']} | "
                         f"{r['over_query']} | {r['emit_gb_per_s']} ({r['query_emit_gb_per_s']}) | {r['today_us']} | {r['today_over_call']} |")
        lines += ["", "| rows, one f32 key | small form: call us | its stages us | large form: call us | its stages us |", "|---|---|---|---|---|"]
        for k, r in res["forms"].items(): lines.append(f"| {k} | {r['small_call_us']} | {r['small_stages_us']} | {r['large_call_us']} | {r['large_stages_us']} |")
        with open(args.readme, "a") as f: f.write("\n".join(lines) + "\n")
    if not ok:
        print("MISMATCH: the sorted rows differ from np.lexsort over the query's rows", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
