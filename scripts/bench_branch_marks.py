#!/usr/bin/env python3
"""Branch steps of a world that defers despawns, measured (profiles/branch_marks/).

The config-5 shape on one GPU: 256 speculative branches x 100 k entities x 8 frames off one snapshot.  The world is the headline particles schema (Transform,
Velocity, Ttl; 60 B per entity) with despawn_particles written as a user system that DEFERS every second entity's despawn (despawn_rollback(), despawn.rs:114-143);
Ttl runs 1..300, so every frame of every branch despawns some.  Timed, interleaved, `--runs` times each:

  a         the marker world through ggrs_hip_fanout_step_branches (one launch for all branches)
  a_newest  ... with GGRS_BRANCH_RETAIN_NEWEST      a_all  ... with GGRS_BRANCH_RETAIN_ALL   (each retained branch keeps a marker record)
  b         the same world, the same step as request lists through ggrs_hip_fanout_step: all such a world could use before
  c         the plain particles world (built-in despawn_particles) through ggrs_hip_fanout_step_branches: its kernel text has no marker code

A run is `--steps` steps, each one call + collect; every step starts from the same snapshot (the world stays at the frame the branches start from), so every
step's gathered table is the same.  After the clock stops each run's LAST table is compared with the oracle: no system of these worlds reads PlayerInputs and
neither has a non-rollback component, so all 256 branches compute the same frames and the oracle (whose twin of the user system is a Python callable) walks the
branch once -- every row of the table must equal that walk.

The script FAILS (exit status 1, after writing its JSON) when a bound is broken:
  - a's median must not exceed b's by more than b's own spread (max - min of its runs);
  - with --parent-c FILE (this script's JSON of `--only c` run from a checkout of the parent commit, on the same box): c's median must not exceed the parent's
    c by more than c's own spread -- c's kernel text is the parent's, so anything else is a host regression.

    python scripts/bench_branch_marks.py --only c --out parent_c.json        # from a checkout of the parent commit (copy this script there): the plain world alone
    python scripts/bench_branch_marks.py --parent-c parent_c.json --out profiles/branch_marks/result.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

TTL_DEFER_SRC = r"""
__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) {
    e.u64(0) -= 1;
    if (e.u64(0) == 0) { if (e.slot & 1) e.despawn_rollback(); else e.despawn(); }
}
"""


def ttl_twin(words, slot, f):
    t = (words[0] - 1) & 0xFFFFFFFFFFFFFFFF
    return [t], (0 if t else (2 if slot & 1 else 1))


def build(world, n, deferring, oracle):
    import numpy as np
    import bevy_ggrs_amd as bg
    import common as cm
    T = world.register_component("Transform", 4, 10)
    V = world.register_component("Velocity", 4, 3)
    L = world.register_component("Ttl", 8, 1)
    world.set_component_default(T, cm.TRANSFORM_DEFAULT)
    world.checksum_component(V, [0, 1, 2])
    world.checksum_component(T, [0, 1, 2])
    world.add_system(bg.SYS_PARTICLES_UPDATE, comp=(T, V), word=(0, 0), fparam=(0.0, -200.0, 0.0))
    if deferring: world.add_custom_system(ttl_twin if oracle else TTL_DEFER_SRC, [(L, 0)], name="despawn_particles")
    else: world.add_system(bg.SYS_TTL_DESPAWN, comp=(L,), word=(0,))
    vel, ttl = cm.synthetic_particles(n, ttl="despawn")
    cm.spawn_particles(world, (T, V, L), n, vel, ttl)
    world.set_depth(9)
    world.handle_requests([bg.AdvanceFrame((0,)), bg.AdvanceFrame((0,))])
    world.set_confirmed(world.frame)                              # every frame of a branch is unconfirmed: despawn_rollback() defers
    return T, V, L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=100_000)
    ap.add_argument("--branches", type=int, default=256)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default="a,a_newest,a_all,b,c")
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-c", default="", help="JSON of `--only c` from the parent commit: c is checked against it")
    args = ap.parse_args()
    import ctypes as C
    import numpy as np
    import __graft_entry__ as ge
    ge.build()
    import bevy_ggrs_amd as bg
    from bevy_ggrs_amd import _ffi
    from bevy_ggrs_amd.fanout import RcclFanout
    from oracle.binding import FLAT, OracleWorld
    n, B, T = args.entities, args.branches, args.frames
    variants = [v for v in args.only.split(",") if v]
    flags_of = {"a": 0, "a_newest": _ffi.BRANCH_RETAIN_NEWEST, "a_all": _ffi.BRANCH_RETAIN_ALL, "c": 0}
    worlds, want = {}, {}
    for deferring in (True, False):
        if not any((v != "c") == deferring for v in variants): continue
        gw = bg.World(n + 64, max_depth=10)
        build(gw, n, deferring, False)
        worlds[deferring] = (gw, RcclFanout(gw, 0, 1, RcclFanout.unique_id()))
        ow = OracleWorld(n + 64, 10, FLAT)
        build(ow, n, deferring, True)
        F = ow.frame
        cs = list(ow.handle_requests([bg.SaveGameState(F)]))
        cs += list(ow.handle_requests([bg.LoadGameState(F)] + [r for i in range(T) for r in (bg.AdvanceFrame((0,)), bg.SaveGameState(F + 1 + i))]))
        want[deferring] = (cs[0], cs[1:])
    inputs = np.zeros((B, T, 1), dtype=np.uint8)

    def run(v):
        deferring = v != "c"
        gw, native = worlds[deferring]
        F = gw.frame
        prefix = [bg.SaveGameState(F)]
        if v == "b":
            reqs = list(prefix)
            for _ in range(B): reqs += [bg.LoadGameState(F)] + [r for i in range(T) for r in (bg.AdvanceFrame((0,)), bg.SaveGameState(F + 1 + i))]
            reqs.append(bg.LoadGameState(F))                    # the list form leaves the world where the branches started, as the branch step does
            arr, keep, _ = gw.build_requests(reqs)
            call = lambda: native.step_raw(arr, len(reqs))
        else:
            pre, keep, _ = gw.build_requests(prefix)
            bs = _ffi.BranchStep()
            bs.prefix, bs.n_prefix, bs.n_branches, bs.n_frames, bs.n_inputs, bs.flags = pre, 1, B, T, 1, _ffi.BRANCH_SAVE_LAST | flags_of[v]
            bs.inputs = inputs.ctypes.data
            call = lambda: native.step_branches(bs)
        tab = None
        for _ in range(args.warmup): call(); tab = native.collect(max(4096, B * T + 1))
        t0 = time.perf_counter()
        for _ in range(args.steps): call(); tab = native.collect(max(4096, B * T + 1))
        dt = time.perf_counter() - t0
        got = [int(p[0]) | (int(p[1]) << 64) for p in tab.reshape(-1, 2)]
        first, per_branch = want[deferring]
        ok = len(got) == 1 + B * T and got[0] == first and all(got[1 + b * T:1 + (b + 1) * T] == per_branch for b in range(B))
        assert gw.frame == F
        return dt / args.steps * 1e3, ok

    res = {v: {"ms_per_step": [], "table_equals_oracle": True} for v in variants}
    for _ in range(args.runs):
        for v in variants:                                       # interleaved: one run of each, then the next round
            ms, ok = run(v)
            res[v]["ms_per_step"].append(round(ms, 4)); res[v]["table_equals_oracle"] &= bool(ok)
    for v in variants:
        ms = res[v]["ms_per_step"]
        res[v]["median_ms"] = round(statistics.median(ms), 4); res[v]["spread_ms"] = round(max(ms) - min(ms), 4)
        res[v]["entity_frames_per_s"] = round(n * B * T / (statistics.median(ms) * 1e-3))
    out = {"shape": {"entities": n, "branches": B, "frames": T, "steps_per_run": args.steps, "warmup": args.warmup, "runs": args.runs}, "variants": res}
    if True in worlds:                                           # what the library says it allocated (ggrs_hip_world_kernel_info)
        info = worlds[True][0].kernel_info()
        if "branch_marker_record_bytes" in info:
            rec, n_rec = int(info["branch_marker_record_bytes"]), int(info["branch_marker_records"])
            out["marker_record_bytes"] = {"per_branch": rec, "records_allocated": n_rec, "allocated": rec * n_rec, "per_slot_of_capacity": round(rec / (n + 64), 3)}
    broken = []
    if "a" in res and "b" in res:
        a, b = res["a"], res["b"]
        ok = a["median_ms"] <= b["median_ms"] + b["spread_ms"]
        out["a_vs_b"] = {"speedup": round(b["median_ms"] / a["median_ms"], 3), "bound_ms": round(b["median_ms"] + b["spread_ms"], 4), "within_bound": ok}
        if not ok: broken.append("a (%.4f ms) is slower than b (%.4f ms) by more than b's spread (%.4f ms)" % (a["median_ms"], b["median_ms"], b["spread_ms"]))
    if args.parent_c and "c" in res:
        pc, c = json.load(open(args.parent_c))["variants"]["c"], res["c"]
        ok = c["median_ms"] <= pc["median_ms"] + c["spread_ms"]
        out["c_vs_parent"] = {"parent": pc, "ratio": round(c["median_ms"] / pc["median_ms"], 4), "bound_ms": round(pc["median_ms"] + c["spread_ms"], 4), "within_bound": ok}
        if not ok: broken.append("c (%.4f ms) is slower than the parent's c (%.4f ms) by more than its own spread (%.4f ms)" % (c["median_ms"], pc["median_ms"], c["spread_ms"]))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(out, indent=1) + "\n")
    for _, native in worlds.values(): native.close()
    assert all(r["table_equals_oracle"] for r in res.values()), "a gathered table differs from the oracle"
    if broken: raise SystemExit("; ".join(broken))


if __name__ == "__main__":
    main()
