#!/usr/bin/env python3
"""What a device scatter costs, measured (profiles/scatter/README.md).  No threshold: nobody has measured this before.

The stress_test world (Transform, Velocity, Ttl: 60 B per entity, 14 words) at `--entities` slots (default 1 M), everyone alive.  Cases:

  (i)    WRITE of Transform.translation (3 x f32) for every live entity -- the rows are a query's output buffer handed back
  (ii)   WRITE of all 14 words for every live entity -- likewise
  (iii)  WRITE of translation to every 32nd entity
  (iv)   INSERT of Velocity (3 words), REMOVE of Velocity and DESPAWN, 4096 rows each (every 16th slot of a range).  Every timed INSERT finds the component
         removed and every timed REMOVE finds it present (the opposite call runs untimed in between); every DESPAWN call has fresh rows: the mask atomics are issued

Each case: `--warmup` calls, then `--calls` calls of ggrs_hip_scatter through the C ABI, each between two HIP events on the world's stream (the record's clear to
the report's copy back); the two launches by themselves from the events the library puts around them (ggrs_dbg_scatter_launch_us).  Two yardsticks that are not
the code under test, on the same device in the same run:

  (a) copy    a hipMemcpyAsync device-to-device that moves as many bytes as the scatter reads plus writes: the slots (twice: both launches read them), the
              mask words and the rows' input words read, the rows' words written -- a copy of half that sum, which reads it once and writes it once
  (b) today   the route through the calls that existed before, host clock (it ends in stream waits).  (i) - (iii): per word download_word over [0, len), a
              numpy merge on the host, upload_word; (iv): 4096 calls of insert_component / remove_component / despawn

After (i) - (iii) the written columns are downloaded and compared with the values: a mismatch is the only thing that makes this script fail.

    python scripts/bench_scatter.py --readme profiles/scatter/README.md
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(stream, fn, warmup, calls, between=None):
    import torch
    us = []
    for k in range(warmup + calls):
        if between: between(k)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream); fn(k); b.record(stream); b.synchronize()
        if k >= warmup: us.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--today-calls", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--readme", default="", help="append the series as a section of this file")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    import torch
    import bevy_ggrs_amd as bg
    import common as cm
    from bevy_ggrs_amd import _ffi
    n, NR = args.entities, 4096
    hip = C.CDLL(None)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]; hip.hipMemcpyAsync.restype = C.c_int
    stream = torch.cuda.Stream()
    w = bg.World(n, max_depth=3, stream=stream.cuda_stream)
    ids = cm.build_particles(w)
    T, V, Lc = ids[:3]
    vel, ttl = cm.synthetic_particles(n)
    cm.spawn_particles(w, ids, n, vel, ttl)
    w.set_depth(3)
    w.handle_requests([bg.AdvanceFrame((0,)), bg.AdvanceFrame((0,))])
    lib, p = w._lib, w._p
    res = {"entities": n, "configs": {}}
    ok = True
    rep = _ffi.ScatterReport()
    units = (n + 63) // 64

    def buffer(words, slots, salt):
        """A device buffer in the query's layout holding `slots` and, per word, a value that says which row it is."""
        lay = w.query_layout(w.query_desc(words, slots=True), slots.size)
        buf = torch.zeros(max(int(lay.total_bytes), 1), dtype=torch.uint8, device="cuda")
        vals = []
        for k, (c, wd) in enumerate(words):
            wb = w._comps[c][1]
            v = (np.float32(salt + k) + (slots % 1000).astype(np.float32)).view(np.uint32) if wb == 4 else np.full(slots.size, 1 << 40, dtype=np.uint64)
            vals.append(v)
            buf[int(lay.col_off[k]):int(lay.col_off[k]) + slots.size * wb].copy_(torch.from_numpy(v.view(np.uint8)).cuda())
        buf[int(lay.slots_off):int(lay.slots_off) + slots.size * 4].copy_(torch.from_numpy(slots.astype(np.uint32).view(np.uint8)).cuda())
        torch.cuda.synchronize()
        return buf, vals

    def scatter(desc, buf, stride, rows):
        rc = lib.ggrs_hip_scatter(p, C.byref(desc), buf.data_ptr(), stride, rows, C.byref(rep))
        assert rc == 0, w._lib.ggrs_hip_last_error(p)

    def launches(fn, between=None):
        assert lib.ggrs_dbg_scatter_launch_us(p, 1, None) == 0
        per = []
        for k in range(args.calls):
            if between: between(k)
            fn(k)
            us = (C.c_double * 2)(); lib.ggrs_dbg_scatter_launch_us(p, 1, us); per.append(list(us))
        lib.ggrs_dbg_scatter_launch_us(p, 0, None)
        return [round(statistics.median(x[k] for x in per), 2) for k in range(2)]

    def copy_us(nbytes):
        half = max(nbytes // 2, 1)
        src, dst = torch.zeros(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        return timed(stream, lambda k: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), half, 3, stream.cuda_stream), args.warmup, args.calls)["median_us"]      # 3: hipMemcpyDeviceToDevice

    def finish(name, r, rows, words, n_masks, mask_rw):
        wbs = [w._comps[c][1] for c, _ in words]
        read = 2 * rows * 4 + rows * sum(wbs) + n_masks * min(rows, units) * 8
        written = rows * sum(wbs) + mask_rw * min(rows, units) * 8
        r.update(rows=rows, words=len(words), bytes_read=read, bytes_written=written, copy_us=copy_us(read + written))
        r["over_copy"] = round(r["median_us"] / r["copy_us"], 2); r["apply_over_copy"] = round(r["apply_us"] / r["copy_us"], 2)
        r["today_over_call"] = round(r["today_us"] / r["median_us"], 1)
        res["configs"][name] = r

    # ---- (i) - (iii): WRITE
    tr = [(T, 0), (T, 1), (T, 2)]
    every = [(T, k) for k in range(10)] + [(V, k) for k in range(3)] + [(Lc, 0)]
    for name, words, slots in (("(i) WRITE translation, every entity", tr, np.arange(n)), ("(ii) WRITE all 14 words, every entity", every, np.arange(n)),
                               ("(iii) WRITE translation, every 32nd entity", tr, np.arange(0, n, 32))):
        desc = w.scatter_desc("write", words)
        buf, vals = buffer(words, slots, 3)
        m = slots.size
        call = lambda k: scatter(desc, buf, m, m)
        r = timed(stream, call, args.warmup, args.calls)
        r["check_us"], r["apply_us"] = launches(call)
        assert (rep.n_applied, rep.n_dead, rep.n_absent) == (m, 0, 0)
        same = all(np.array_equal(w.download_word(c, k, 0, n)[slots], v) for (c, k), v in zip(words, vals))
        ok = ok and same
        r["matches_values"] = bool(same)
        host = []
        for _ in range(args.today_calls):
            t0 = time.perf_counter()
            for (c, k), v in zip(words, vals):
                col = w.download_word(c, k, 0, n); col[slots] = v; w.upload_word(c, k, 0, col)
            host.append((time.perf_counter() - t0) * 1e6)
        r["today_us"] = round(statistics.median(host), 1)
        finish(name, r, m, words, 2, 0)                                            # (alive and one presence word per unit read; no mask written)
        del buf

    # ---- (iv): INSERT, REMOVE, DESPAWN of 4096 rows
    vw = [(V, 0), (V, 1), (V, 2)]
    slots = np.arange(0, NR * 16, 16)
    ins, rem = w.scatter_desc("insert", vw), w.scatter_desc("remove", comps=[V])
    ibuf, ivals = buffer(vw, slots, 5)
    sbuf, _ = buffer([], slots, 0)
    do_ins, do_rem = (lambda k: scatter(ins, ibuf, NR, NR)), (lambda k: scatter(rem, sbuf, NR, NR))
    for name, fn, undo, words, mask_rw, today in (
            ("(iv) INSERT Velocity, 4096 rows", do_ins, do_rem, vw, 1, lambda: [w.insert_component(V, int(s), np.array([v[i] for v in ivals], dtype=np.uint32)) for i, s in enumerate(slots)]),
            ("(iv) REMOVE Velocity, 4096 rows", do_rem, do_ins, [], 1, lambda: [w.remove_component(V, int(s)) for s in slots])):
        r = timed(stream, fn, args.warmup, args.calls, between=undo)
        r["check_us"], r["apply_us"] = launches(fn, between=undo)
        assert rep.n_applied == NR
        undo(0)
        t0 = time.perf_counter(); today(); w.synchronize()
        r["today_us"] = round((time.perf_counter() - t0) * 1e6, 1)
        finish(name, r, NR, words, 2, mask_rw)
    do_ins(0)
    des = w.scatter_desc("despawn")
    total = args.warmup + 2 * args.calls
    assert NR * 4 * (2 + total) <= n, "the world is too small for fresh rows per despawn call"
    fresh = [buffer([], np.arange(NR * 4 * (1 + j), NR * 4 * (2 + j), 4), 0)[0] for j in range(total)]      # (every 4th slot of a range of its own)
    r = timed(stream, lambda k: scatter(des, fresh[k], NR, NR), args.warmup, args.calls)
    assert rep.n_applied == NR
    r["check_us"], r["apply_us"] = launches(lambda k: scatter(des, fresh[args.warmup + args.calls + k], NR, NR))
    assert rep.n_applied == NR
    t0 = time.perf_counter()
    for s in np.arange(1, NR * 16, 16): w.despawn(int(s))
    w.synchronize()
    r["today_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    finish("(iv) DESPAWN, 4096 rows", r, NR, [], 1, 1)
    w.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(res, indent=1) + "\n")
    if args.readme:
        lines = ["", f"### Measured: {n} slots of the stress_test world, everyone alive, {args.calls} calls after {args.warmup}", "",
                 "| case | rows | bytes read + written | median us per call (min .. max) | check / apply launch us | (a) copy of the same bytes us | call / (a) | apply / (a) | (b) today's route us | (b) / call |",
                 "|---|---|---|---|---|---|---|---|---|---|"]
        for k, r in res["configs"].items():
            lines.append(f"| {k} | {r['rows']} | {r['bytes_read']} + {r['bytes_written']} | {r['median_us']} ({r['min_us']} .. {r['max_us']}) | {r['check_us']} / {r['apply_us']} | "
                         f"{r['copy_us']} | {r['over_copy']} | {r['apply_over_copy']} | {r['today_us']} | {r['today_over_call']} |")
        with open(args.readme, "a") as f: f.write("\n".join(lines) + "\n")
    if not ok:
        print("MISMATCH: a written column differs from the values scattered into it", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
