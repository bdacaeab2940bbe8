#!/usr/bin/env python3
"""What the peer index costs and what it buys, measured (profiles/peer_index/README.md).  No threshold: nobody has measured this before.

1. build   the build cost per AdvanceWorld: a world of one key column and one system that reads its own bucket's count, keys constant, at `--sizes` slots x
           `--buckets` n_buckets, keys uniform and everyone in ONE bucket.  Every launch of the `advance` class (the publish, then the k_ix_* launches, in
           submission order) by HIP events (ggrs_hip_profile_read_launches): the median of `--windows` windows of `--ticks` AdvanceWorlds after `--warmup`, with the
           spread; the launch count; the one-bucket / uniform ratio per size and n_buckets, and per launch position -- which pass pays.
2. buys    the crowd world of tests/peer_index_common.py at `--crowd` slots, about 8 members per cell, against the same arithmetic written the only way a world
           without the index allows: a loop over all len slots through e.peer(i) with the cell test inside.  Wall-clock per tick around blocking
           handle_requests([AdvanceFrame, SaveGameState]) calls, windows alternating between the two worlds; their checksums, which must be equal.  The brute-force
           form is quadratic: it is run at these sizes only.
3. tick    the crowd tick at `--big` slots split into publish, index build and request-group launch (kernel time per class and launch position), next to the
           follow world of scripts/bench_peer_reads.py (peer reads, no index) at the same sizes.

    python scripts/bench_peer_index.py --out profiles/peer_index/result.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
COUNT_SRC = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) = e.bucket(e.peer(e.slot).u32(0)).count(); }"


def med(xs): return round(float(statistics.median(xs)), 2)


def spread(xs): return [round(float(min(xs)), 2), round(float(max(xs)), 2)]


def advance_windows(w, ticks, windows, reqs):
    """Per window: the `advance` launches of `ticks` lists, as microseconds per launch POSITION inside a list (publish first), summed and per position."""
    per_list, totals, by_pos = None, [], []
    for _ in range(windows):
        w.profile_enable(True)
        for _t in range(ticks): w.handle_requests(reqs())
        w.synchronize()
        us = list(w.profile_launches("advance"))
        w.profile_enable(False)
        assert us and len(us) % ticks == 0, (len(us), ticks)
        per_list = len(us) // ticks
        totals.append(sum(us) / ticks)
        by_pos.append([statistics.median(us[k::per_list]) for k in range(per_list)])
    return {"launches_per_advance": per_list, "us_per_advance_median": med(totals), "us_per_advance_spread": spread(totals),
            "us_by_position_median": [med([b[k] for b in by_pos]) for k in range(per_list)]}


def build_cost(args):
    import numpy as np
    import bevy_ggrs_amd as bg
    out = []
    for n in args.sizes:
        for nb in args.buckets:
            row = {"slots": n, "n_buckets": nb}
            for pattern in ("uniform", "one_bucket"):
                w = bg.World(n + 64, max_depth=2)
                K = w.register_component("Key", 4, 1); O = w.register_component("Out", 4, 1)
                w.checksum_component(O, [0])
                w.register_peer_index(K, 0, nb)
                w.add_custom_system(COUNT_SRC, [(O, 0)], name="count", peers=[(K, 0)])
                i = np.arange(n, dtype=np.int64)
                key = ((i * 2654435761) % nb if pattern == "uniform" else np.full(n, nb // 2)).astype(np.uint32)
                w.spawn(n, {K: [key], O: [np.zeros(n, dtype=np.uint32)]})
                w.set_depth(2); w.set_synctest_check_distance(-1)
                reqs = lambda: [bg.AdvanceFrame((0,))]
                for _ in range(args.warmup): w.handle_requests(reqs())
                row[pattern] = advance_windows(w, args.ticks, args.windows, reqs)
                start, slots = w.peer_index()
                row[pattern]["n_indexed"] = int(start[-1]); row[pattern]["largest_bucket"] = int(np.diff(start.astype(np.int64)).max())
                w.close()
            row["one_bucket_over_uniform"] = round(row["one_bucket"]["us_per_advance_median"] / row["uniform"]["us_per_advance_median"], 3)
            row["one_bucket_over_uniform_by_position"] = [round(a / b, 2) if b else None for a, b in zip(row["one_bucket"]["us_by_position_median"], row["uniform"]["us_by_position_median"])]
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def what_it_buys(args):
    import bevy_ggrs_amd as bg
    import peer_index_common as pc
    out = []
    for n in args.crowd:
        gw = max(2, int(round((n / 8.0) ** 0.5)))
        worlds, sums = {}, {}
        for kind in ("index", "brute"):
            w = bg.World(n + 64, max_depth=2)
            ids = pc.build_crowd(w, gw, gw, brute_len=n if kind == "brute" else 0)
            pc.spawn_crowd(w, ids, n, gw, gw, 11, span=gw)
            w.set_depth(2); w.set_synctest_check_distance(-1)
            worlds[kind] = w; sums[kind] = []
        tick = lambda w, f: w.handle_requests([bg.AdvanceFrame((0,)), bg.SaveGameState(f)])
        F = {k: 0 for k in worlds}
        us = {k: [] for k in worlds}
        for k, w in worlds.items():
            for _ in range(args.warmup): F[k] += 1; sums[k] += tick(w, F[k])
        for _ in range(args.windows):
            for k, w in worlds.items():                                  # alternating
                t0 = time.perf_counter()
                for _t in range(args.crowd_ticks): F[k] += 1; sums[k] += tick(w, F[k])
                w.synchronize()
                us[k].append((time.perf_counter() - t0) / args.crowd_ticks * 1e6)
        row = {"slots": n, "grid": gw, "members_per_cell": round(n / gw / gw, 2), "checksums_equal": sums["index"] == sums["brute"], "frames_compared": len(sums["index"])}
        for k in worlds: row[k] = {"us_per_tick_median": med(us[k]), "us_per_tick_spread": spread(us[k])}
        row["brute_over_index"] = round(row["brute"]["us_per_tick_median"] / row["index"]["us_per_tick_median"], 2)
        for w in worlds.values(): w.close()
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def tick_split(args):
    import bevy_ggrs_amd as bg
    import peer_index_common as pc
    import peer_reads_common as pr
    out = []
    for n in args.big:
        row = {"slots": n}
        for kind in ("crowd", "follow"):
            w = bg.World(n + 64, max_depth=2)
            if kind == "crowd":
                gw = min(255, max(2, int(round((n / 8.0) ** 0.5))))
                ids = pc.build_crowd(w, gw, gw); pc.spawn_crowd(w, ids, n, gw, gw, 12, span=gw)
                row["grid"] = gw
            else:
                ids = pr.build_follow(w); pr.spawn_follow(w, ids, n)
            w.set_depth(2); w.set_synctest_check_distance(-1)
            reqs = lambda: [bg.AdvanceFrame((0,))]
            for _ in range(args.warmup): w.handle_requests(reqs())
            r = advance_windows(w, args.ticks, args.windows, reqs)
            w.profile_enable(True)
            for _t in range(args.ticks): w.handle_requests(reqs())
            w.synchronize()
            tk = sorted(w.profile_launches("tick"))
            w.profile_enable(False)
            pos = r["us_by_position_median"]
            row[kind] = {"publish_us": pos[0], "index_build_us": round(sum(pos[1:]), 2), "index_launches": len(pos) - 1, "advance_class": r,
                         "request_group_launch_us_median": med(tk), "request_group_launch_us_spread": spread(tk)}
            w.close()
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ints = lambda s: [int(x) for x in s.split(",") if x]
    ap.add_argument("--sizes", type=ints, default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--buckets", type=ints, default=[255, 4096, 65535])
    ap.add_argument("--crowd", type=ints, default=[4096, 16384])
    ap.add_argument("--big", type=ints, default=[100_000, 1_000_000])
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--crowd-ticks", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parts", default="build,buys,tick")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    os.environ["GGRS_JIT_SPECIALISE_AFTER"] = "0"                       # neither world straddles a kernel switch
    import __graft_entry__ as ge
    ge.build()
    out = {"shape": {k: getattr(args, k) for k in ("sizes", "buckets", "crowd", "big", "ticks", "crowd_ticks", "windows", "warmup")}}
    if "build" in args.parts: out["build_cost"] = build_cost(args)
    if "buys" in args.parts: out["what_it_buys"] = what_it_buys(args)
    if "tick" in args.parts: out["tick_split"] = tick_split(args)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
