#!/usr/bin/env python3
"""What a state diff costs, measured (profiles/state_diff/README.md).  No threshold: nobody has measured this before.

The stress_test world (Transform, Velocity, Ttl: 60 B per entity, 14 columns) at `--entities` slots (default 1 M) runs a few SyncTest ticks; then two ADJACENT
ring frames are compared in three forms:

  full      ggrs_hip_diff_frames without flags: every rollback row of both blocks is read (one AdvanceWorld apart: every live entity differs)
  trust     the same with GGRS_DIFF_TRUST_VERSIONS: the columns no system writes carry the same row version on both sides and are skipped on the host
  zero      a frame against a ggrs_hip_snapshot_copy of itself (ggrs_hip_diff_block): every row is read, nothing differs, nothing is emitted

Each form: `--warmup` calls, then `--calls` calls, each between two HIP events on the world's stream (first command to last: the counter memset, the launches, the
report's copy back).  On the same device, in the same run, the yardstick: a hipMemcpyAsync device-to-device of one block's rollback rows (60 B x slots), timed the same
way.  The expectation to TEST, not a bound: the full compare takes about the time of reading both blocks once, twice the copy's read side.

    python scripts/bench_state_diff.py --readme profiles/state_diff/README.md
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys

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
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-entries", type=int, default=64)
    ap.add_argument("--grids", type=int, nargs="*", default=[], help="also time the full compare with at most this many workgroups per launch")
    ap.add_argument("--out", default="")
    ap.add_argument("--readme", default="", help="append the series as a section of this file")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import torch
    import bevy_ggrs_amd as bg
    import common as cm
    n, D = args.entities, args.depth
    stream = torch.cuda.Stream()
    w = bg.World(n, max_depth=D + 2, stream=stream.cuda_stream)
    ids = cm.build_particles(w)
    vel, ttl = cm.synthetic_particles(n)
    cm.spawn_particles(w, ids, n, vel, ttl)
    drv = cm.SyncTestDriver(w, D, max_prediction=D + 1)
    for _ in range(6): drv.tick((0,))
    fb = w.frame - 1; fa = fb - 1
    assert w.has_snapshot(fa) and w.has_snapshot(fb)
    w.diff(fa, fb)                                                   # (deferred Saves land in their slots before anything is timed)
    res = {"entities": n, "frames": [fa, fb], "bytes_per_slot": cm.schema_bytes_per_entity(), "forms": {}}

    # the timed calls go straight through the C ABI with buffers made once: what a Rust or C++ caller pays, no Python between the events
    from bevy_ggrs_amd import _ffi
    rep, ents = _ffi.DiffReport(), (_ffi.DiffEntry * max(1, args.max_entries))()
    lib, p = w._lib, w._p

    def frames(cap, flags=0):
        def fn(): assert lib.ggrs_hip_diff_frames(p, fa, fb, flags, C.byref(rep), ents if cap else None, cap) == 0
        return fn

    def form(name, fn):
        fn()
        r = timed(stream, fn, args.warmup, args.calls)
        cols, bps, masks, _ = (int(x) for x in re.search(r"compared (\d+) columns \((\d+) bytes per slot and side\) and (\d+) masks over (\d+) units", w.kernel_info()["state_diff"]).groups())
        r.update(n_entities=int(rep.n_entities), entries=int(rep.n_entries), columns=cols, bytes_read=2 * (bps * n + masks * ((n + 63) // 64) * 8))
        r["read_gb_per_s"] = round(r["bytes_read"] / r["median_us"] / 1e3, 1)
        res["forms"][name] = r

    form("full", frames(args.max_entries))
    form("full, counts only", frames(0))                             # one launch: no scan, no emit
    form("trust", frames(args.max_entries, _ffi.DIFF_TRUST_VERSIONS))
    blk = w.snapshot_copy(fb)

    def zero(): assert lib.ggrs_hip_diff_block(p, fb, blk.data_ptr(), 0, C.byref(rep), ents, args.max_entries) == 0
    form("zero", zero)
    # the launch geometry (ggrs_dbg_set_diff_grid: at most that many workgroups per launch; 0 = the library's choice): the full compare under each
    res["grids"] = {}
    for g in args.grids:
        assert lib.ggrs_dbg_set_diff_grid(p, g) == 0
        res["grids"][g] = timed(stream, frames(args.max_entries), args.warmup, args.calls)["median_us"]
    lib.ggrs_dbg_set_diff_grid(p, 0)
    # the yardstick: one block's rollback rows, device to device, on the same stream
    nbytes = res["bytes_per_slot"] * n
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    src.zero_(); torch.cuda.synchronize()
    hip = C.CDLL(None)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]; hip.hipMemcpyAsync.restype = C.c_int

    def copy():
        assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream) == 0      # 3: hipMemcpyDeviceToDevice
    res["copy"] = dict(timed(stream, copy, args.warmup, args.calls), bytes=nbytes)
    res["copy"]["read_gb_per_s"] = round(nbytes / res["copy"]["median_us"] / 1e3, 1)
    for k, r in res["forms"].items(): r["over_copy"] = round(r["median_us"] / res["copy"]["median_us"], 2)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(res, indent=1) + "\n")
    if args.readme:
        lines = ["", f"### Measured: {n} slots, frames {fa} and {fb} of a SyncTest session (check distance {D}), {args.calls} calls after {args.warmup}, max_entries {args.max_entries}", "",
                 "| form | median us per call (min .. max) | differing entities | columns compared | bytes read per call | GB/s read | time / copy |", "|---|---|---|---|---|---|---|"]
        for k, r in res["forms"].items():
            lines.append(f"| {k} | {r['median_us']} ({r['min_us']} .. {r['max_us']}) | {r['n_entities']} | {r['columns']} | {r['bytes_read']} | {r['read_gb_per_s']} | {r['over_copy']} |")
        c = res["copy"]
        lines.append(f"| hipMemcpyAsync D2D of one block's rows | {c['median_us']} ({c['min_us']} .. {c['max_us']}) | | | {c['bytes']} read + as many written | {c['read_gb_per_s']} | 1 |")
        if res["grids"]: lines += ["", "Full compare, median us per call by the cap on workgroups per launch: " + ", ".join(f"{g}: {us}" for g, us in res["grids"].items())]
        with open(args.readme, "a") as f: f.write("\n".join(lines) + "\n")
    w.close()


if __name__ == "__main__":
    main()
