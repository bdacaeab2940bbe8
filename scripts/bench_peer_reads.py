#!/usr/bin/env python3
"""What peer bindings cost, measured (profiles/peer_reads/README.md).  No threshold: nobody has measured this before.

The follow world of tests/peer_reads_common.py at `--entities` slots (default 100 k), SyncTest check distance `--depth` (default 8):

  peer  system A reads its target's Pos through e.peer(slot) (ggrs_hip_add_custom_system_peers): the peer view, one k_publish_peers launch ahead of every
        request group that holds an AdvanceWorld, one AdvanceWorld per group
  own   the same world, the same arithmetic, the same columns stored, A's peer reads replaced by reads of its OWN Pos: no view, no publish launch,
        groups of any length

Both on the same commit, alternating, `--runs` runs of `--ticks` ticks each after `--warmup` ticks (the shapes of a steady tick are warm by then; specialised
copies are switched off for both worlds so that neither run straddles a kernel switch).  Wall-clock per tick around blocking ggrs_hip_handle_requests calls,
then ONE instrumented pass per world (ggrs_hip_profile_*): kernel time and launches per class, every launch's duration (ggrs_hip_profile_read_launches), the
bytes the launches were asked to move.  The publish launches are counted in the `advance` class, the request-group launches in `tick`.

    python scripts/bench_peer_reads.py --out profiles/peer_reads/result.json
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
    import numpy as np
    import bevy_ggrs_amd as bg
    import peer_reads_common as pc
    w = bg.World(n + 64, max_depth=depth + 1)
    if kind == "peer":
        ids = pc.build_follow(w)
    else:
        P = w.register_component("Pos", 4, 2); T = w.register_component("Target", 8, 1); V = w.register_component("Vel", 4, 2); H = w.register_component("Hp", 4, 1)
        w.set_component_default(H, np.array([1000], dtype=np.uint32))
        w.checksum_component(P, [0, 1]); w.checksum_component(T, [0]); w.checksum_component(V, [0, 1])
        w.add_custom_system(pc.FOLLOW_OWN_SRC, [(V, 0), (V, 1), (T, 0), (P, 0), (P, 1)], iparam=(n,), fparam=(pc.GAIN,), name="follow_own")
        w.add_custom_system(pc.INTEGRATE_SRC, [(P, 0), (P, 1), (V, 0), (V, 1)], name="integrate")
        w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(H,), word=(0,), iparam=(1, 0))
        ids = (P, T, V, H)
    pc.spawn_follow(w, ids, n)
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=100_000)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    os.environ["GGRS_JIT_SPECIALISE_AFTER"] = "0"
    import __graft_entry__ as ge
    ge.build()
    import common as cm
    n, D = args.entities, args.depth
    worlds = {k: build(k, n, D) for k in ("peer", "own")}
    drv = {k: cm.SyncTestDriver(w, D, max_prediction=D + 1) for k, w in worlds.items()}
    for k in worlds:
        for t in range(args.warmup): drv[k].tick((t & 3,))
        worlds[k].synchronize()
    res = {k: {"us_per_tick": []} for k in worlds}
    for _ in range(args.runs):
        for k, w in worlds.items():                                  # alternating: one run of each, then the next round
            t0 = time.perf_counter()
            for t in range(args.ticks): drv[k].tick((t & 3,))
            w.synchronize()
            res[k]["us_per_tick"].append(round((time.perf_counter() - t0) / args.ticks * 1e6, 2))
    for k, w in worlds.items():                                      # the instrumented pass, after the clocks stopped
        w.profile_enable(True)
        w.host_timeline(1)
        for t in range(60): drv[k].tick((t & 3,))
        w.synchronize()
        prof, byts, tl = w.profile_read(), w.profile_bytes(), w.host_timeline(0)
        r = res[k]
        r["median_us_per_tick"] = statistics.median(r["us_per_tick"]); r["spread_us"] = round(max(r["us_per_tick"]) - min(r["us_per_tick"]), 2)
        r["profiled_ticks"] = 60
        r["classes"] = {}
        for cls in ("tick", "advance", "checksum"):
            ms, launches = prof[cls]
            if not launches: continue
            us = sorted(w.profile_launches(cls))
            r["classes"][cls] = {"launches_per_tick": round(launches / 60, 2), "kernel_us_per_tick": round(ms * 1e3 / 60, 2), "launch_us_median": round(float(statistics.median(us)), 2),
                                 "launch_us_min": round(float(us[0]), 2), "launch_us_p90": round(float(us[int(len(us) * 0.9)]), 2), "bytes_per_tick": int(byts[cls] // 60)}
        r["host_launch_calls_per_tick"] = round(tl["launches"] / 60, 2); r["host_launch_call_us_per_tick"] = round(tl["launch_call_us"] / 60, 2)
        r["kernel_info"] = {x: w.kernel_info().get(x) for x in ("group_caps", "peer_view", "kernarg_bytes", "checksum_fold")}
        w.profile_enable(False)
        r["equal_final_len"] = w.len
    out = {"shape": {"entities": n, "check_distance": D, "ticks_per_run": args.ticks, "warmup": args.warmup, "runs": args.runs}, "worlds": res,
           "peer_over_own": round(res["peer"]["median_us_per_tick"] / res["own"]["median_us_per_tick"], 3)}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
