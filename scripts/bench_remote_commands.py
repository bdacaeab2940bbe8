#!/usr/bin/env python3
"""What remote bindings cost, measured (profiles/remote_commands/README.md).  No threshold: nobody has measured this before.

Two worlds of Hp, Target and Stun{ticks, seed} at `--entities` slots (default 1 M), links (i * 389 + 17) % n with every 13th at slot 0 and every 10th out of range
(tests/peer_effects_common.py strike_links), SyncTest check distance `--depth` (default 8):

  remote  Stun absent at spawn.  `countdown` (own binding Hp, command binding Stun with REMOVE) counts a stunned entity down and removes Stun at 1; `striker`,
          registered last, sends e.send_insert(target, Stun) when (slot + frame) % 3 == 0 (ggrs_hip_add_custom_system_remote): one inbox word per slot, one
          k_apply_remote launch per frame
  fx      the same arithmetic with Stun ALWAYS present (ticks == 0 stands for "absent") and written through effects: MAX_U of the default ticks into Stun.ticks,
          OR of the default seed into Stun.seed (ggrs_hip_add_custom_system_effects): two inbox columns, one k_apply_effects launch per frame.  This world uses
          nothing this feature adds, so `--root <a checkout of the parent commit> --only fx` times the parent's library on it

Both alternating, `--runs` runs of `--ticks` ticks each after `--warmup` ticks (specialised copies are switched off for both worlds so that neither run straddles a
kernel switch).  Wall-clock per tick around blocking ggrs_hip_handle_requests calls, then ONE instrumented pass per world (ggrs_hip_profile_*): launches and kernel
time of the request-group class and of the advance class (the applies).

    python scripts/bench_remote_commands.py --out profiles/remote_commands/1m.json --readme profiles/remote_commands/README.md
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(kind, n, depth):
    import numpy as np
    import bevy_ggrs_amd as bg
    import remote_commands_common as rc
    w = bg.World(n + 64, max_depth=depth + 1)
    H = w.register_component("Hp", 4, 1); T = w.register_component("Target", 8, 1); S = w.register_component("Stun", 4, 2)
    w.set_component_default(S, np.array(rc.STUN_DEFAULT, dtype=np.uint32))
    for c, words in ((H, [0]), (T, [0]), (S, [0, 1])): w.checksum_component(c, words)
    hp = ((np.arange(n) * 37 + 11) % 101).astype(np.uint32)
    if kind == "remote":
        w.add_custom_system(rc.COUNTDOWN_SRC, [(H, 0)], name="countdown", commands=[(S, bg.CMD_REMOVE)])
        w.add_custom_system(rc.STRIKER_STUN_SRC, [(T, 0)], name="striker", remote=[(S, bg.REMOTE_INSERT)])
        w.spawn(n, {H: [hp], T: [rc.strike_links(n)]})
    else:
        w.add_custom_system(rc.COUNTDOWN_OWN_SRC, [(H, 0), (S, 0)], name="countdown_own")
        w.add_custom_system(rc.STRIKER_FX_SRC, [(T, 0)], name="striker_fx", effects=[(S, 0, bg.EFFECT_MAX_U), (S, 1, bg.EFFECT_OR)])
        w.spawn(n, {H: [hp], T: [rc.strike_links(n)], S: [np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)]})
    return w, (H, T, S)


README = """# Remote structural commands (remote bindings): what they cost

`ggrs_hip_add_custom_system_remote` (DESIGN §3.10) lets a user-written system despawn other entities and insert / remove their components: one inbox word per
slot, one no-return `global_atomic_or` per send, one `k_apply_remote` launch behind every request group that holds an AdvanceWorld.

## 1. The remote-stun world against the same arithmetic through effects

Method: `python scripts/bench_remote_commands.py --out profiles/remote_commands/1m.json --readme profiles/remote_commands/README.md`.
{shape}
Two worlds on the same commit, alternating; then one instrumented pass of 60 ticks per world.

- `remote`: `Stun{{ticks, seed}}` absent at spawn; `countdown` removes it at 1 through a command binding (§3.7), `striker`, registered last, sends
  `e.send_insert(target, Stun)` when `(slot + frame) % 3 == 0`.
- `fx`: `Stun` always present (`ticks == 0` stands for "absent"), the striker sends `MAX_U` of the default ticks and `OR` of the default seed through effect
  bindings (§3.6). This world uses nothing the feature adds; `--root <parent checkout> --only fx` times the parent commit's library on it.

By launch count a frame of either world is one group launch plus one apply.

{numbers}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=1_000_000)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default="", help="remote or fx: one world only")
    ap.add_argument("--root", default=HERE, help="the checkout whose library is timed (default: this one)")
    ap.add_argument("--parent-json", default="", help="the --out of a `--root <parent> --only fx` run: its fx time goes into the README")
    ap.add_argument("--out", default="")
    ap.add_argument("--readme", default="")
    args = ap.parse_args()
    os.environ["GGRS_JIT_SPECIALISE_AFTER"] = "0"
    root = os.path.abspath(args.root)
    sys.path.insert(0, os.path.join(HERE, "tests")); sys.path.insert(0, os.path.join(root, "tests")); sys.path.insert(0, root)
    import __graft_entry__ as ge
    ge.build()
    import common as cm
    n, D = args.entities, args.depth
    kinds = [args.only] if args.only else ["remote", "fx"]
    built = {k: build(k, n, D) for k in kinds}
    worlds = {k: b[0] for k, b in built.items()}
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
    P = 60
    for k, w in worlds.items():                                      # the instrumented pass, after the clocks stopped
        w.profile_enable(True)
        for t in range(P): drv[k].tick((t % 3,))
        w.synchronize()
        prof = w.profile_read()
        r = res[k]
        r["median_us_per_tick"] = statistics.median(r["us_per_tick"]); r["spread_us"] = round(max(r["us_per_tick"]) - min(r["us_per_tick"]), 2)
        r["us_per_step"] = round(r["median_us_per_tick"] / (D + 1), 2)                    # a SyncTest tick at check distance D simulates D + 1 frames
        for cls in ("tick", "advance"):
            ms, launches = prof[cls]
            us = sorted(w.profile_launches(cls))
            r[cls + "_class"] = {"launches_per_tick": round(launches / P, 2), "kernel_us_per_tick": round(ms * 1e3 / P, 2),
                                 "launch_us_median": round(float(statistics.median(us)), 2) if us else None}
        info = w.kernel_info()
        r["kernel_info"] = {x: info.get(x) for x in ("group_caps", "remote_inbox", "effect_inbox", "command_bindings", "kernarg_bytes")}
        w.profile_enable(False)
        S = built[k][1][2]
        on = w.present_mask(S, n) & w.alive_mask(n)
        r["stunned_at_end"] = int((on & (w.download_word(S, 0, 0, n) > 0)).sum())
    out = {"root": "this tree" if root == HERE else "another checkout (--root)", "shape": {"entities": n, "check_distance": D, "ticks_per_run": args.ticks, "warmup": args.warmup, "runs": args.runs},
           "worlds": res}
    if len(kinds) == 2: out["remote_over_fx"] = round(res["remote"]["median_us_per_tick"] / res["fx"]["median_us_per_tick"], 3)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(out, indent=1) + "\n")
    if args.readme and len(kinds) == 2:
        parent = None
        if args.parent_json and os.path.exists(args.parent_json): parent = json.load(open(args.parent_json))["worlds"]["fx"]
        shape = (f"{n} slots, SyncTest check distance {D} ({D + 1} simulated frames per tick), blocking `ggrs_hip_handle_requests`, specialised copies off; "
                 f"{args.runs} runs of {args.ticks} ticks each after {args.warmup} warm-up ticks.")
        rows = ["| world | us per tick (median of the runs; each run) | us per step | group launches / tick, kernel us | apply launches / tick, kernel us |", "|---|---|---|---|---|"]
        def row(name, r):
            return (f"| {name} | {r['median_us_per_tick']} ({', '.join(str(x) for x in r['us_per_tick'])}) | {r['us_per_step']} | {r['tick_class']['launches_per_tick']}, "
                    f"{r['tick_class']['kernel_us_per_tick']} | {r['advance_class']['launches_per_tick']}, {r['advance_class']['kernel_us_per_tick']} |")
        rows.append(row("`remote`", res["remote"])); rows.append(row("`fx`", res["fx"]))
        rows.append(row("`fx` on the parent commit's library", parent) if parent else "| `fx` on the parent commit's library | not measured | | | |")
        numbers = "Numbers (one MI355X, one box, one session):\n\n" + "\n".join(rows) + f"\n\n`remote` / `fx` = {out['remote_over_fx']} per tick.  Stunned entities at the end: {res['remote']['stunned_at_end']} (`remote`), {res['fx']['stunned_at_end']} (`fx`).\n"
        with open(args.readme, "w") as f: f.write(README.format(shape=shape, numbers=numbers))


if __name__ == "__main__":
    main()
