#!/usr/bin/env python3
"""What deterministic float sums into a device resource cost, measured (profiles/float_sums/README.md).  No threshold: nobody has measured this before.

The flock world of tests/sums_common.py at 100 k and 1 M slots (`--entities`), SyncTest check distance `--depth` (default 7):

  sums     Centre{sx, sy} (f32 sums), Energy{e} (f64 sum), Census{alive: u32 ADD}; `steer` reads last frame's Centre, `reset` (a resource system) starts the frame's
           sums, `tally` and `skew` sum: per-lane accumulators, a DPP ladder of float adds per wave, ONE plain store per wave and word into the partial arrays,
           k_apply_sums behind every launch that simulates a frame
  plain    (a) the same world with the e.sum_* calls and the sum bindings removed: the same resources, systems and columns, the u32 reducer kept
  ureduce  (b) the same world with the sums replaced by u32 ADD reducers of the values' bits (reduce bindings: one no-return atomic per wave and word into the striped
           inbox): what a fixed-point workaround pays

All three on the same tree in one session, alternating, `--runs` runs of `--ticks` ticks each after `--warmup` ticks (specialised copies are switched off so that no
run straddles a kernel switch).  Wall-clock per tick around blocking ggrs_hip_handle_requests calls that end in a synchronise, then ONE instrumented pass per world
(ggrs_hip_profile_*): launches per tick over every kernel class, and for the sums world the duration of every k_apply_sums launch (the `advance` class holds the
applies in submission order: k_apply_reduces, k_apply_sums, alternating).

    python scripts/bench_sums.py --readme profiles/float_sums/README.md
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
KINDS = ("sums", "plain", "ureduce")


def build(kind, n, depth):
    import bevy_ggrs_amd as bg
    import sums_common as sc
    w = bg.World(n + 64, max_depth=depth + 1)
    ids = sc.build_flock(w, variant=kind, fuse_step=0)               # nobody dies: every world keeps every slot busy
    sc.spawn_flock(w, ids, n)
    return w


def measure(n, args):
    import common as cm
    D = args.depth
    worlds = {k: build(k, n, D) for k in KINDS}
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
        r["group_launch_us"] = round(prof["tick"][0] * 1e3 / max(1, prof["tick"][1]), 2)
        if k == "sums":
            applies = list(w.profile_launches("advance"))
            mine = applies[1::2]                                     # k_apply_reduces, k_apply_sums, k_apply_reduces, ..
            r["k_apply_sums_us"] = round(statistics.median(mine), 2) if mine else None
            r["k_apply_reduces_us"] = round(statistics.median(applies[0::2]), 2) if applies else None
            r["sum_partials"] = w.kernel_info().get("sum_partials", "")
        w.profile_enable(False)
    med = {k: res[k]["median_us_per_tick"] for k in KINDS}
    return {"entities": n, "worlds": res, "sums_over_plain": round(med["sums"] / med["plain"], 3), "sums_over_ureduce": round(med["sums"] / med["ureduce"], 3)}


def register_lines():
    """VGPR / SGPR / scratch of the flock world's generic and steady kernels, with and without the sum bindings (compiled for gfx950 here; no device involved)."""
    import bevy_ggrs_amd as bg
    import sums_common as sc
    from test_resources_text import _build
    rows = []
    for form, steady in (("generic", False), ("steady", True)):
        for which in ("sums", "plain"):
            w = bg.World(600, max_depth=8, flags=bg.GGRS_WORLD_LAYOUT_ONLY); sc.build_flock(w, variant=which)
            res, asm = _build(w.generated_kernel_source(steady=steady, compile=True))
            rows.append(f"| {which} | {form} | {res['vgpr_count']} | {res['sgpr_count']} | {res['private_segment_fixed_size']} | {asm.count('global_atomic')} |")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--depth", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--readme", default="", help="append the series as a section of this file")
    ap.add_argument("--registers-only", action="store_true", help="print the register lines and stop (needs no device)")
    args = ap.parse_args()
    os.environ["GGRS_JIT_SPECIALISE_AFTER"] = "0"
    import __graft_entry__ as ge
    ge.build()
    regs = ["| world | kernel | VGPRs | SGPRs | scratch bytes | global_atomic instructions |", "|---|---|---|---|---|---|"] + register_lines()
    if args.registers_only:
        print("\n".join(regs)); return
    out = {"shape": {"check_distance": args.depth, "ticks_per_run": args.ticks, "warmup": args.warmup, "runs": args.runs}, "sizes": [measure(n, args) for n in args.entities]}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(out, indent=1) + "\n")
    if args.readme:
        lines = ["", f"### Measured: check distance {args.depth}, {args.runs} runs of {args.ticks} ticks each, the three worlds alternating in one session, generic kernels", "",
                 "| slots | world | us per tick, each run | median ms per step | launches per tick | group launch us |", "|---|---|---|---|---|---|"]
        for s in out["sizes"]:
            for k in KINDS:
                r = s["worlds"][k]
                lines.append(f"| {s['entities']} | {k} | {r['us_per_tick']} | {r['ms_per_step']} | {r['launches_per_tick']} | {r['group_launch_us']} |")
            lines.append(f"| {s['entities']} | sums / plain | {s['sums_over_plain']} | | | |")
            lines.append(f"| {s['entities']} | sums / ureduce | {s['sums_over_ureduce']} | | | |")
            r = s["worlds"]["sums"]
            lines.append(f"| {s['entities']} | k_apply_sums, median us per launch | {r['k_apply_sums_us']} | (k_apply_reduces beside it: {r['k_apply_reduces_us']}) | | |")
        have = open(args.readme).read() if os.path.exists(args.readme) else ""
        if not all(row in have for row in regs[2:]): lines += ["", "### Registers (compiled for gfx950)", ""] + regs
        with open(args.readme, "a") as f: f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
