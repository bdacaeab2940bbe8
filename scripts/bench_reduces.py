#!/usr/bin/env python3
"""What entity systems that reduce into a device resource cost, measured (profiles/resource_reduces/README.md).  No threshold: nobody has measured this before.

The census world of tests/reduces_common.py at 100 k and 1 M slots (`--entities`), SyncTest check distance `--depth` (default 7):

  census  Census{alive: ADD, flags: OR}, Low{hp: MIN_U}, Total{hp_sum: ADD}; `look` reads last frame's count, `reset` (a resource system) starts the frame's count,
          `wound` and `count` reduce: per-lane accumulators, a DPP ladder per wave, one no-return atomic per wave and word into the striped inbox, k_apply_reduces
          behind every launch that simulates a frame
  plain   the same world with the reduce_* calls and the reduce bindings removed: the same resources, systems and columns, request groups of many frames

Both on the same tree, alternating, `--runs` runs of `--ticks` ticks each after `--warmup` ticks (specialised copies are switched off for both worlds so that
neither run straddles a kernel switch).  Wall-clock per tick around blocking ggrs_hip_handle_requests calls, then ONE instrumented pass per world
(ggrs_hip_profile_*): launches per tick over every kernel class.  The number of inbox lines comes from the environment variable BENCH_REDUCE_STRIPES (1..64, default 64; handed to the
library before seal): run the script once per value for the stripe series.

    BENCH_REDUCE_STRIPES=64 python scripts/bench_reduces.py --readme profiles/resource_reduces/README.md
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def build(kind, n, depth):
    import bevy_ggrs_amd as bg
    import reduces_common as rd
    w = bg.World(n + 64, max_depth=depth + 1)
    if w._lib.ggrs_dbg_set_reduce_stripes(w._p, int(os.environ.get("BENCH_REDUCE_STRIPES", "64"))) != 0: raise SystemExit("BENCH_REDUCE_STRIPES must be 1..64")
    ids = rd.build_census(w, plain=kind == "plain", fuse_step=0)      # nobody dies: both worlds keep every slot busy
    rd.spawn_census(w, ids, n)
    return w


def measure(n, args):
    import common as cm
    D = args.depth
    worlds = {k: build(k, n, D) for k in ("census", "plain")}
    drv = {k: cm.SyncTestDriver(w, D, max_prediction=D + 1) for k, w in worlds.items()}
    for k in worlds:
        for t in range(args.warmup): drv[k].tick((t % 3,))
        worlds[k].synchronize()
    res = {k: {"us_per_tick": []} for k in worlds}
    for _ in range(args.runs):
        for k, w in worlds.items():                                  # alternating: one run of each, then the next round
            t0 = time.perf_counter()
            for t in range(args.ticks): drv[k].tick((t % 3,))
            w.synchronize()
            res[k]["us_per_tick"].append(round((time.perf_counter() - t0) / args.ticks * 1e6, 2))
    P = 40
    for k, w in worlds.items():                                      # the instrumented pass, after the clocks stopped
        w.profile_enable(True)
        for t in range(P): drv[k].tick((t % 3,))
        w.synchronize()
        prof = w.profile_read()
        r = res[k]
        r["median_us_per_tick"] = statistics.median(r["us_per_tick"]); r["spread_us"] = round(max(r["us_per_tick"]) - min(r["us_per_tick"]), 2)
        r["ms_per_step"] = round(r["median_us_per_tick"] / (D + 1) / 1e3, 5)              # a SyncTest tick at check distance D simulates D + 1 frames
        r["launches_per_tick"] = round(sum(v[1] for v in prof.values()) / P, 2)
        r["launches"] = {c: v[1] for c, v in prof.items()}
        r["reduce_inbox"] = w.kernel_info().get("reduce_inbox", "")
        w.profile_enable(False)
    return {"entities": n, "worlds": res, "census_over_plain": round(res["census"]["median_us_per_tick"] / res["plain"]["median_us_per_tick"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--depth", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--readme", default="", help="append the series as a section of this file")
    args = ap.parse_args()
    os.environ["GGRS_JIT_SPECIALISE_AFTER"] = "0"
    stripes = int(os.environ.get("BENCH_REDUCE_STRIPES", "64"))
    import __graft_entry__ as ge
    ge.build()
    out = {"shape": {"check_distance": args.depth, "ticks_per_run": args.ticks, "warmup": args.warmup, "runs": args.runs, "stripes": stripes}, "sizes": [measure(n, args) for n in args.entities]}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(out, indent=1) + "\n")
    if args.readme:
        lines = ["", f"### Measured: {stripes} inbox lines, check distance {args.depth}, {args.runs} runs of {args.ticks} ticks each, alternating, generic kernels", "",
                 "| slots | world | us per tick, each run | median ms per step | launches per tick |", "|---|---|---|---|---|"]
        for s in out["sizes"]:
            for k in ("census", "plain"):
                r = s["worlds"][k]
                lines.append(f"| {s['entities']} | {k} | {r['us_per_tick']} | {r['ms_per_step']} | {r['launches_per_tick']} |")
            lines.append(f"| {s['entities']} | census / plain | {s['census_over_plain']} | | |")
        with open(args.readme, "a") as f: f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
