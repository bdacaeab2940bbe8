#!/usr/bin/env python3
"""What command bindings cost, measured (profiles/structural_commands/README.md).  No threshold: nobody has measured this before.

The stun world of tests/commands_common.py at `--entities` slots (default 1 M), SyncTest check distance `--depth` (default 8):

  cmd  Stun absent at spawn; the system inserts and removes it through a command binding (ggrs_hip_add_custom_system_commands): Stun's presence bit is a
       register, its mask word is rebuilt with one ballot per Save and stored with every Save
  own  the same world with Stun always present and the same arithmetic written through ordinary bindings (ticks == 0 stands for "absent"): the masks never
       change, the same three columns are stored with every Save

Both on the same commit, alternating, `--runs` runs of `--ticks` ticks each after `--warmup` ticks (specialised copies are switched off for both worlds so that
neither run straddles a kernel switch).  Wall-clock per tick around blocking ggrs_hip_handle_requests calls, then ONE instrumented pass per world
(ggrs_hip_profile_*): kernel time and launches of the request-group class, every launch's duration, the bytes the launches were asked to move.  The VGPR /
scratch line of both kernels comes from the code objects' notes (hiprtc + llvm-readelf, as tests/test_commands_text.py does), where the tools are present.

    python scripts/bench_commands.py --out profiles/structural_commands/1m.json
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
    import numpy as np
    import bevy_ggrs_amd as bg
    import commands_common as cc
    w = bg.World(n + 64, max_depth=depth + 1)
    hp = ((np.arange(n) * 37 + 11) % 101).astype(np.uint32)
    if kind == "cmd":
        ids = cc.build_stun(w)
        w.spawn(n, {ids[0]: [hp]})
    else:
        H = w.register_component("Hp", 4, 1); S = w.register_component("Stun", 4, 2)
        w.checksum_component(H, [0]); w.checksum_component(S, [0, 1])
        w.add_custom_system(cc.STUN_OWN_SRC, [(H, 0), (S, 0), (S, 1)], name="stun_own")
        w.spawn(n, {H: [hp], S: [np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)]})
    return w


def resources(w):
    """{vgpr_count, private_segment_fixed_size, ..} of the world's generic kernel, from the code object's notes; None without the tools."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=1_000_000)
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
    worlds = {k: build(k, n, D) for k in ("cmd", "own")}
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
        prof, byts = w.profile_read(), w.profile_bytes()
        r = res[k]
        r["median_us_per_tick"] = statistics.median(r["us_per_tick"]); r["spread_us"] = round(max(r["us_per_tick"]) - min(r["us_per_tick"]), 2)
        r["ms_per_step"] = round(r["median_us_per_tick"] / 1e3 / (D + 1), 5)              # a SyncTest tick at check distance D simulates D + 1 frames
        ms, launches = prof["tick"]
        us = sorted(w.profile_launches("tick"))
        r["tick_class"] = {"launches_per_tick": round(launches / P, 2), "kernel_us_per_tick": round(ms * 1e3 / P, 2), "launch_us_median": round(float(statistics.median(us)), 2),
                           "launch_us_min": round(float(us[0]), 2), "launch_us_p90": round(float(us[int(len(us) * 0.9)]), 2), "bytes_per_launch": int(byts["tick"] // max(1, launches))}
        r["kernel_info"] = {x: w.kernel_info().get(x) for x in ("group_caps", "command_bindings", "kernarg_bytes", "checksum_fold", "lazy_live_block", "deferred_saves", "value_tags")}
        r["kernel_resources"] = resources(w)
        w.profile_enable(False)
        r["present_at_end"] = int((w.present_mask(1, n) & w.alive_mask(n)).sum())
    out = {"shape": {"entities": n, "check_distance": D, "ticks_per_run": args.ticks, "warmup": args.warmup, "runs": args.runs}, "worlds": res,
           "cmd_over_own": round(res["cmd"]["median_us_per_tick"] / res["own"]["median_us_per_tick"], 3)}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f: f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
