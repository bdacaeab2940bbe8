#!/usr/bin/env python3
"""What effect bindings cost, measured (profiles/peer_effects/README.md).  No threshold: nobody has measured this before.

The strike world of tests/peer_effects_common.py at `--entities` slots (default 100 k), SyncTest check distance `--depth` (default 8), with `--links`:

  spread  links (i * 389 + 17) % n, every tenth out of range, every thirteenth on slot 0
  slot0   every link on slot 0: every send of a frame lands on ONE inbox word per column

  fx   the striker sends to its target through e.send_* (ggrs_hip_add_custom_system_effects): the inbox, one k_apply_effects launch behind every request
       group that holds an AdvanceWorld, groups that end on their one AdvanceWorld
  own  the same world, the same arithmetic, the same columns stored, the striker writing its OWN Hp, Flags, Low and Score: no inbox, no apply launch, groups
       of any length

Both on the same commit, alternating, `--runs` runs of `--ticks` ticks each after `--warmup` ticks (specialised copies are switched off for both worlds so that
neither run straddles a kernel switch).  Wall-clock per tick around blocking ggrs_hip_handle_requests calls, then ONE instrumented pass per world
(ggrs_hip_profile_*): kernel time and launches per class, every launch's duration, the bytes the launches were asked to move.  The request-group launches are
counted in the `tick` class, the apply launches in `advance` (the strike world reads no peers: nothing else is in that class).

    python scripts/bench_peer_effects.py --entities 100000 --links spread --out profiles/peer_effects/100k_spread.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def build(kind, n, depth, links):
    import numpy as np
    import bevy_ggrs_amd as bg
    import peer_effects_common as pc
    w = bg.World(n + 64, max_depth=depth + 1)
    if kind == "fx":
        ids = pc.build_strike(w)
    else:
        P = w.register_component("Pos", 4, 2); T = w.register_component("Target", 8, 1); F = w.register_component("Fuse", 4, 1); H = w.register_component("Hp", 4, 1)
        G = w.register_component("Flags", 4, 1); L = w.register_component("Low", 4, 1); S = w.register_component("Score", 8, 1)
        w.set_component_default(F, np.array([1000], dtype=np.uint32)); w.set_component_default(L, np.array([50], dtype=np.uint32))
        for c, words in ((P, [0, 1]), (T, [0]), (F, [0]), (H, [0]), (G, [0]), (L, [0]), (S, [0])): w.checksum_component(c, words)
        w.add_system(bg.SYS_SAT_SUB_DESPAWN, comp=(F,), word=(0,), iparam=(1, 0))
        w.add_custom_system(pc.MOVE_SRC, [(P, 0), (P, 1)], name="mover")
        w.add_custom_system(pc.STRIKE_OWN_SRC, [(T, 0), (P, 0), (P, 1), (H, 0), (G, 0), (L, 0), (S, 0)], iparam=(n,), name="strike_own")
        ids = (P, T, F, H, G, L, S)
    pc.spawn_strike(w, ids, n, links=None if links == "spread" else np.zeros(n, dtype=np.uint64))
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=100_000)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--links", choices=("spread", "slot0"), default="spread")
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
    worlds = {k: build(k, n, D, args.links) for k in ("fx", "own")}
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
    P = 60
    for k, w in worlds.items():                                      # the instrumented pass, after the clocks stopped
        w.profile_enable(True)
        w.host_timeline(1)
        for t in range(P): drv[k].tick((t & 3,))
        w.synchronize()
        prof, byts, tl = w.profile_read(), w.profile_bytes(), w.host_timeline(0)
        r = res[k]
        r["median_us_per_tick"] = statistics.median(r["us_per_tick"]); r["spread_us"] = round(max(r["us_per_tick"]) - min(r["us_per_tick"]), 2)
        r["profiled_ticks"] = P
        r["classes"] = {}
        for cls, what in (("tick", "request groups"), ("advance", "apply launches"), ("checksum", "finalize")):
            ms, launches = prof[cls]
            if not launches: continue
            us = sorted(w.profile_launches(cls))
            r["classes"][cls] = {"what": what, "launches_per_tick": round(launches / P, 2), "kernel_us_per_tick": round(ms * 1e3 / P, 2), "launch_us_median": round(float(statistics.median(us)), 2),
                                 "launch_us_min": round(float(us[0]), 2), "launch_us_p90": round(float(us[int(len(us) * 0.9)]), 2), "bytes_per_tick": int(byts[cls] // P)}
        r["host_launch_calls_per_tick"] = round(tl["launches"] / P, 2); r["host_launch_call_us_per_tick"] = round(tl["launch_call_us"] / P, 2)
        r["kernel_info"] = {x: w.kernel_info().get(x) for x in ("group_caps", "effect_inbox", "kernarg_bytes", "checksum_fold")}
        w.profile_enable(False)
        r["final_len"] = w.len
    out = {"shape": {"entities": n, "check_distance": D, "links": args.links, "ticks_per_run": args.ticks, "warmup": args.warmup, "runs": args.runs}, "worlds": res,
           "fx_over_own": round(res["fx"]["median_us_per_tick"] / res["own"]["median_us_per_tick"], 3)}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
