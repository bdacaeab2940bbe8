#!/usr/bin/env python3
"""What value bindings cost, measured (profiles/remote_values/README.md).  No threshold: nobody has measured this before.

Three worlds of Hp, Target, Power, Burn{dps, ticks, source} and Mark{id} at each of `--entities` slots (default 100 k and 1 M), links (i * 389 + 17) % n with every
13th at slot 0 and every 10th out of range (tests/peer_effects_common.py strike_links), SyncTest check distance `--depth` (default 8):

  value   the brand world of tests/remote_values_common.py: torch sends Burn with ITS OWN dps / ticks / source through two value bindings, the tagger Mark and Burn
          through two more (ggrs_hip_add_custom_system_values): per sender the staged words at its own slot, one 64-bit atomic max and one atomic or
  insert  THE SAME WORLD with e.send_insert of the registered default wherever `value` sends a value: the parent commit's feature, the reference for the cost
  fx      the workaround value bindings remove: Burn ALWAYS present (ticks == 0 stands for "absent"), written through integer effects -- MAX_U of the dps bits and
          of the ticks, OR of the source -- with the same sending conditions; no Mark, no remove, no despawn (effects cannot express them)

The worlds alternate, `--runs` runs of `--ticks` ticks each after `--warmup` ticks (specialised copies are switched off so that no run straddles a kernel switch).
Wall-clock per tick around blocking ggrs_hip_handle_requests calls, then ONE instrumented pass per world (ggrs_hip_profile_*): launches and kernel time of the
request-group class (the group launch) and of the advance class (the applies: k_apply_remote / k_apply_effects).

    python scripts/bench_remote_values.py --out profiles/remote_values/bench.json --readme profiles/remote_values/README.md
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTDOWN_OWN_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    e.u32(0) = e.u32(0) + (ggrs_u32)f.input[0];
    if (e.u32(1) >= 1u) e.u32(1) -= 1u;
}
"""
# bindings 0 = Target, 1 = Power; effect bindings 0 = Burn.dps (MAX_U of the float's bits), 1 = Burn.ticks (MAX_U), 2 = Burn.source (OR)
TORCH_FX_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u64 t = e.u64(0), n = (ggrs_u64)f.iparam[0];
    const ggrs_u32 k = (ggrs_u32)e.slot + (ggrs_u32)f.frame;
    if (k % 3u == 0u) { e.send_u32(t, 0, __float_as_uint((float)e.u32(1) * 0.5f)); e.send_u32(t, 1, 2u + k % 5u); e.send_u32(t, 2, (ggrs_u32)e.slot); }
    if (k % 4u == 1u) { const ggrs_u64 t1 = (t + 1ull) % n; e.send_u32(t1, 0, __float_as_uint((float)e.u32(1) * 0.25f)); e.send_u32(t1, 1, 3u); e.send_u32(t1, 2, (ggrs_u32)e.slot); }
    if (k % 5u == 2u) { e.send_u32(t, 0, 0x3fc00000u); e.send_u32(t, 1, 3u); }
}
"""
TAGGER_FX_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {
    const ggrs_u64 t = e.u64(0);
    const ggrs_u32 k = (ggrs_u32)e.slot + (ggrs_u32)f.frame;
    if (k % 6u == 0u) { e.send_u32(t, 0, __float_as_uint((float)e.u32(1) * 2.0f)); e.send_u32(t, 1, 9u); e.send_u32(t, 2, (ggrs_u32)e.slot); }
}
"""


def build(kind, n, depth):
    import numpy as np
    import bevy_ggrs_amd as bg
    import remote_values_common as rv
    w = bg.World(n + 64, max_depth=depth + 1)
    if kind in ("value", "insert"):
        ids = rv.build_brand(w, n, values=kind == "value")
        rv.spawn_brand(w, ids, n)
        return w, ids
    H = w.register_component("Hp", 4, 1); T = w.register_component("Target", 8, 1); P = w.register_component("Power", 4, 1); B = w.register_component("Burn", 4, 3)
    for c, words in ((H, [0]), (T, [0]), (P, [0]), (B, [0, 1, 2])): w.checksum_component(c, words)
    fx = [(B, 0, bg.EFFECT_MAX_U), (B, 1, bg.EFFECT_MAX_U), (B, 2, bg.EFFECT_OR)]
    w.add_custom_system(COUNTDOWN_OWN_SRC, [(H, 0), (B, 1)], name="countdown_own")
    w.add_custom_system(TORCH_FX_SRC, [(T, 0), (P, 0)], iparam=(n, 0), name="torch_fx", effects=fx)
    w.add_custom_system(TAGGER_FX_SRC, [(T, 0), (P, 0)], name="tagger_fx", effects=fx)
    i = np.arange(n)
    z = np.zeros(n, dtype=np.uint32)
    w.spawn(n, {H: [((i * 37 + 11) % 101).astype(np.uint32)], T: [rv.strike_links(n)], P: [(3 + (i * 7) % 29).astype(np.uint32)], B: [z, z.copy(), z.copy()]})
    return w, (H, T, P, B)


README = """# Remote inserts that carry the sender's value (value bindings): what they cost

`ggrs_hip_add_custom_system_values` (DESIGN §3.13) lets a user-written system insert a component into another entity with its own words: per sender the staged
words go to a payload array at its own slot (plain coalesced stores), the key `(g + 1) << 40 | (slot + 1)` into the target's winner word with one no-return
`global_atomic_umax_x2`, and one `global_atomic_or` of the component's value bit into the target's remote inbox word; `k_apply_remote` reads the winner word,
gathers the winner's words and zeroes the winner word.  No launch is added.

Method: `python scripts/bench_remote_values.py --out profiles/remote_values/bench.json --readme profiles/remote_values/README.md`.
{shape}
Three worlds on the same commit, alternating; then one instrumented pass of 60 ticks per world.

- `value`: the brand world of `tests/remote_values_common.py` -- four value bindings (torch: Burn twice; tagger: Mark and Burn), a default insert, a remove, a despawn.
- `insert`: the same world with `e.send_insert` of the registered default wherever `value` sends a value. That is the parent commit's feature: the reference.
- `fx`: the always-present-plus-effects workaround: `Burn` on every entity (`ticks == 0` stands for "absent"), written with `MAX_U` / `MAX_U` / `OR`; no Mark, no
  remove, no despawn. Its result is NOT the same (two words of one Burn can come from two senders): it is the cost of what users did before.

Expected, to be confirmed or refuted: the group launch costs two atomics and `n_words` coalesced stores more per sender than `insert`; the apply costs one `u64`
load and `n_words` gathered loads more per hit target.

{numbers}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--readme", default="")
    args = ap.parse_args()
    os.environ["GGRS_JIT_SPECIALISE_AFTER"] = "0"
    sys.path.insert(0, os.path.join(HERE, "tests")); sys.path.insert(0, HERE)
    import __graft_entry__ as ge
    ge.build()
    import common as cm
    D = args.depth
    kinds = ["value", "insert", "fx"]
    out = {"shape": {"check_distance": D, "ticks_per_run": args.ticks, "warmup": args.warmup, "runs": args.runs}, "sizes": {}}
    P = 60
    for n in args.entities:
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
            r["kernel_info"] = {x: info.get(x) for x in ("group_caps", "remote_inbox", "value_inbox", "effect_inbox", "kernarg_bytes")}
            w.profile_enable(False)
            B = built[k][1][3]
            on = w.present_mask(B, n) & w.alive_mask(n)
            r["burning_at_end"] = int((on & (w.download_word(B, 1, 0, n) > 0)).sum())
        out["sizes"][str(n)] = {"worlds": res, "value_over_insert": round(res["value"]["median_us_per_tick"] / res["insert"]["median_us_per_tick"], 3),
                                "value_over_fx": round(res["value"]["median_us_per_tick"] / res["fx"]["median_us_per_tick"], 3)}
        del drv, worlds, built
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(out, indent=1) + "\n")
    if args.readme:
        shape = (f"{', '.join(str(n) for n in args.entities)} slots, SyncTest check distance {D} ({D + 1} simulated frames per tick), blocking `ggrs_hip_handle_requests`, specialised copies off; "
                 f"{args.runs} runs of {args.ticks} ticks each after {args.warmup} warm-up ticks.")
        rows = ["| slots | world | us per tick (median of the runs; each run) | us per step | group launches / tick, kernel us, us per launch | apply launches / tick, kernel us, us per launch |", "|---|---|---|---|---|---|"]
        for n in args.entities:
            for k in kinds:
                r = out["sizes"][str(n)]["worlds"][k]
                rows.append(f"| {n} | `{k}` | {r['median_us_per_tick']} ({', '.join(str(x) for x in r['us_per_tick'])}) | {r['us_per_step']} | {r['tick_class']['launches_per_tick']}, "
                            f"{r['tick_class']['kernel_us_per_tick']}, {r['tick_class']['launch_us_median']} | {r['advance_class']['launches_per_tick']}, {r['advance_class']['kernel_us_per_tick']}, "
                            f"{r['advance_class']['launch_us_median']} |")
        ratios = "; ".join(f"{n} slots: `value` / `insert` = {out['sizes'][str(n)]['value_over_insert']}, `value` / `fx` = {out['sizes'][str(n)]['value_over_fx']}" for n in args.entities)
        numbers = "Numbers (one MI355X, one box, one session):\n\n" + "\n".join(rows) + f"\n\nPer tick: {ratios}.\n"
        with open(args.readme, "w") as f: f.write(README.format(shape=shape, numbers=numbers))


if __name__ == "__main__":
    main()
