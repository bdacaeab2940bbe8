#!/usr/bin/env python3
"""What a checksum-parts call costs, measured (profiles/checksum_parts/README.md).  No threshold: nobody has measured this before.

The stress_test world (Transform, Velocity, Ttl: 60 B per entity; two checksummed components of three f32 words each: 24 hashed bytes per entity) at `--entities`
slots (default 1 M) runs a few SyncTest ticks; then, on the same device in the same run:

  parts, frame     ggrs_hip_checksum_parts of a ring frame
  parts, live      ... of the live world (GGRS_DIFF_LIVE)
  parts, block     ggrs_hip_checksum_parts_block of a ggrs_hip_snapshot_copy of that frame (one more header read)
  diff             ggrs_hip_diff_frames of two adjacent frames, 64 entries (what the state diff costs on this box)
  copy             hipMemcpyAsync device to device of the hashed rows (24 B x slots)

Each form: `--warmup` calls, then `--calls` calls, each between two HIP events on the world's stream (first command to last: the accumulators' memset, the two launches,
the copy back).  The calls go straight through the C ABI with buffers made once.  The launches by themselves are read with HIP events the library puts around them
(ggrs_dbg_parts_launch_us), in calls of their own so that the call-level times carry no event records.  Expectation to TEST, not a bound: the hashing launch is bound
by its SeaHash diffuses, not by HBM.

    python scripts/bench_checksum_parts.py --readme profiles/checksum_parts/README.md
"""
import argparse
import ctypes as C
import json
import os
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
    ap.add_argument("--grids", type=int, nargs="*", default=[], help="also time the hashing launch with at most this many workgroups")
    ap.add_argument("--out", default="")
    ap.add_argument("--readme", default="", help="append the series as a section of this file")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import torch
    import bevy_ggrs_amd as bg
    import common as cm
    from bevy_ggrs_amd import _ffi
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
    returned = dict(drv.all_checksums)
    p = w.checksum_parts(fb)                                         # (deferred Saves land in their slots before anything is timed)
    assert p.checksum == returned[fb] and list(p.parts) == ["Transform", "Velocity", "Entity"], str(p)
    hashed = 24
    res = {"entities": n, "frames": [fa, fb], "hashed_bytes_per_slot": hashed, "forms": {}}
    lib, wp = w._lib, w._p
    rep, parts = _ffi.PartsReport(), (_ffi.ChecksumPart * _ffi.MAX_PARTS)()
    drep, dents = _ffi.DiffReport(), (_ffi.DiffEntry * 64)()
    blk = w.snapshot_copy(fb)

    def frame(): assert lib.ggrs_hip_checksum_parts(wp, fb, C.byref(rep), parts, _ffi.MAX_PARTS) == 0
    def live(): assert lib.ggrs_hip_checksum_parts(wp, _ffi.DIFF_LIVE, C.byref(rep), parts, _ffi.MAX_PARTS) == 0
    def block(): assert lib.ggrs_hip_checksum_parts_block(wp, blk.data_ptr(), C.byref(rep), parts, _ffi.MAX_PARTS) == 0
    def diff(): assert lib.ggrs_hip_diff_frames(wp, fa, fb, 0, C.byref(drep), dents, 64) == 0

    nbytes = hashed * n
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    src.zero_(); torch.cuda.synchronize()
    hip = C.CDLL(None)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]; hip.hipMemcpyAsync.restype = C.c_int

    def copy(): assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream) == 0      # 3: hipMemcpyDeviceToDevice

    # two rounds, the forms alternating, so that a drift of the device's clock falls on all of them alike; the second round is reported, the first shows the spread
    forms = (("parts, frame", frame), ("parts, live", live), ("parts, block", block), ("diff", diff), ("copy", copy))
    first = {}
    for rnd in range(2):
        for name, fn in forms:
            fn()
            r = timed(stream, fn, args.warmup, args.calls)
            if rnd == 0: first[name] = r["median_us"]
            else: res["forms"][name] = dict(r, first_round_median_us=first[name])
    for name, r in res["forms"].items(): r["over_copy"] = round(r["median_us"] / res["forms"]["copy"]["median_us"], 2)
    masks = 3 * ((n + 63) // 64) * 8
    res["bytes_read_per_call"] = nbytes + masks
    # the launches by themselves
    us = (C.c_double * 2)()
    assert lib.ggrs_dbg_parts_launch_us(wp, 1, None) == 0
    hs, fs = [], []
    for i in range(args.warmup + args.calls):
        frame(); lib.ggrs_dbg_parts_launch_us(wp, 1, us)
        if i >= args.warmup: hs.append(us[0]); fs.append(us[1])
    res["launches"] = {"k_parts_hash_us": {"median": round(statistics.median(hs), 2), "min": round(min(hs), 2), "max": round(max(hs), 2)},
                       "k_parts_finish_us": {"median": round(statistics.median(fs), 2), "min": round(min(fs), 2), "max": round(max(fs), 2)}}
    res["launches"]["k_parts_hash_gb_per_s"] = round(res["bytes_read_per_call"] / res["launches"]["k_parts_hash_us"]["median"] / 1e3, 1)
    res["grids"] = {}
    for g in args.grids:
        assert lib.ggrs_dbg_set_parts_grid(wp, g) == 0
        xs = []
        for i in range(args.warmup + args.calls):
            frame(); lib.ggrs_dbg_parts_launch_us(wp, 1, us)
            if i >= args.warmup: xs.append(us[0])
        res["grids"][g] = round(statistics.median(xs), 2)
    lib.ggrs_dbg_set_parts_grid(wp, 0); lib.ggrs_dbg_parts_launch_us(wp, 0, None)
    res["copy_gb_per_s_read"] = round(nbytes / res["forms"]["copy"]["median_us"] / 1e3, 1)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(res, indent=1) + "\n")
    if args.readme:
        L = res["launches"]
        lines = ["", f"### Measured: {n} slots, frame {fb} of a SyncTest session (check distance {D}), {args.calls} calls after {args.warmup}, second of two alternating rounds", "",
                 "| form | median us per call (min .. max) | median of the first round | time / copy |", "|---|---|---|---|"]
        for k, r in res["forms"].items(): lines.append(f"| {k} | {r['median_us']} ({r['min_us']} .. {r['max_us']}) | {r['first_round_median_us']} | {r['over_copy']} |")
        lines += ["", f"The launches by themselves (HIP events around each, {args.calls} calls): `k_parts_hash` {L['k_parts_hash_us']['median']} us ({L['k_parts_hash_us']['min']} .. {L['k_parts_hash_us']['max']}), "
                      f"{res['bytes_read_per_call']} bytes read = {L['k_parts_hash_gb_per_s']} GB/s; `k_parts_finish` {L['k_parts_finish_us']['median']} us ({L['k_parts_finish_us']['min']} .. {L['k_parts_finish_us']['max']}).  "
                      f"The copy reads {nbytes} bytes (and writes as many) at {res['copy_gb_per_s_read']} GB/s."]
        if res["grids"]: lines += ["", "`k_parts_hash`, median us by the cap on its workgroups (`ggrs_dbg_set_parts_grid`): " + ", ".join(f"{g}: {u}" for g, u in res["grids"].items())]
        with open(args.readme, "a") as f: f.write("\n".join(lines) + "\n")
    w.close()


if __name__ == "__main__":
    main()
