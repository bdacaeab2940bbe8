#!/usr/bin/env python3
"""What device-resident resources cost, measured (profiles/device_resources/README.md).  No threshold: nobody has measured this before.

The clock world of tests/resources_common.py at 100 k and 1 M slots (`--entities`), SyncTest check distance `--depth` (default 8):

  clock  three resources (Clock{ticks, seed}, Wind{x}, Big{acc}), the resource system `tick` between two entity systems that read resources, every resource checksummed
  plain  the same world with `tick` removed and `before` / `drift` reading constants: no resource, the same columns stored with every Save

Both on the same commit, alternating, `--runs` runs of `--ticks` ticks each after `--warmup` ticks (specialised copies are switched off for both worlds so that
neither run straddles a kernel switch).  Wall-clock per tick around blocking ggrs_hip_handle_requests calls, then ONE instrumented pass per world
(ggrs_hip_profile_*): kernel time and launches of the request-group class, every launch's duration.  The VGPR / SGPR / scratch line of both kernels comes from the
code objects' notes (hiprtc + llvm-readelf, as tests/test_resources_text.py does), where the tools are present.

    python scripts/bench_resources.py --readme profiles/device_resources/README.md
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
OPTS = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def build(kind, n, depth):
    import bevy_ggrs_amd as bg
    import resources_common as rc
    w = bg.World(n + 64, max_depth=depth + 1)
    ids = rc.build_clock(w, plain=kind == "plain", fuse_step=0)      # nobody dies: both worlds keep every slot busy
    rc.spawn_clock(w, ids, n)
    return w


def resources(w):
    """{vgpr_count, sgpr_count, private_segment_fixed_size, ..} of the world's generic kernel, from the code object's notes; None without the tools."""
    if not os.path.exists(READELF): return None
    try: rtc = C.CDLL("libhiprtc.so")
    except OSError: return None
    src = w.generated_kernel_source()
    prog = C.c_void_p()
    if rtc.hiprtcCreateProgram(C.byref(prog), src.encode(), b"k.hip", 0, None, None) != 0: return None
    if rtc.hiprtcCompileProgram(prog, len(OPTS), (C.c_char_p * len(OPTS))(*OPTS)) != 0: return None
    n = C.c_size_t(); rtc.hiprtcGetCodeSize(prog, C.byref(n)); code = C.create_string_buffer(n.value); rtc.hiprtcGetCode(prog, code)
    with tempfile.NamedTemporaryFile(suffix=".hsaco") as f:
        f.write(code.raw); f.flush()
        notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|sgpr_count):\s+(\d+)", notes)}


def measure(n, args):
    import common as cm
    D = args.depth
    worlds = {k: build(k, n, D) for k in ("clock", "plain")}
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
        r["us_per_step"] = round(r["median_us_per_tick"] / (D + 1), 3)                    # a SyncTest tick at check distance D simulates D + 1 frames
        ms, launches = prof["tick"]
        us = sorted(w.profile_launches("tick"))
        r["tick_class"] = {"launches_per_tick": round(launches / P, 2), "kernel_us_per_tick": round(ms * 1e3 / P, 2), "launch_us_median": round(float(statistics.median(us)), 2),
                           "launch_us_min": round(float(us[0]), 2)}
        r["launches"] = {c: v[1] for c, v in prof.items()}
        r["kernel_resources"] = resources(w)
        w.profile_enable(False)
    return {"entities": n, "worlds": res, "clock_over_plain": round(res["clock"]["median_us_per_tick"] / res["plain"]["median_us_per_tick"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--readme", default="", help="append the series as a section of this file")
    args = ap.parse_args()
    os.environ["GGRS_JIT_SPECIALISE_AFTER"] = "0"
    import __graft_entry__ as ge
    ge.build()
    out = {"shape": {"check_distance": args.depth, "ticks_per_run": args.ticks, "warmup": args.warmup, "runs": args.runs}, "sizes": [measure(n, args) for n in args.entities]}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(out, indent=1) + "\n")
    if args.readme:
        lines = ["", f"### Measured: check distance {args.depth}, {args.runs} runs of {args.ticks} ticks each, alternating, generic kernels", "",
                 "| slots | world | us per tick, each run | median us per step | launches per tick | kernel us per tick | VGPR / SGPR / scratch |", "|---|---|---|---|---|---|---|"]
        for s in out["sizes"]:
            for k in ("clock", "plain"):
                r = s["worlds"][k]; kr = r["kernel_resources"] or {}
                lines.append(f"| {s['entities']} | {k} | {r['us_per_tick']} | {r['us_per_step']} | {r['tick_class']['launches_per_tick']} | {r['tick_class']['kernel_us_per_tick']} | "
                             f"{kr.get('vgpr_count')} / {kr.get('sgpr_count')} / {kr.get('private_segment_fixed_size')} |")
            lines.append(f"| {s['entities']} | clock / plain | {s['clock_over_plain']} | | | | |")
        with open(args.readme, "a") as f: f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
