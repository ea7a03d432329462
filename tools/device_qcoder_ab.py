#!/usr/bin/env python3
"""A/B of where effort-0 images are entropy coded: mode 0 (host coder threads), 1 (device rANS stage), 2 (shared), each
at several values of n_host_buffers -- in mode 1 that is the number of lanes that can be in flight.  One process, one
library, a fresh context per leg, the modes alternating, `--runs` runs each.  Image sets: `--big` SYN-1 frames of 4096^2
per call (the bench.py --effort 0 step) and `--small` frames of 512^2.

Per leg: wall time and Mpixel/s, the process's CPU seconds (resource.getrusage), the stats call's symbols / kernel_ms as
the lane rate, and whether the first, the last and a middle stream equal mode 0's.  Writes one JSON document.

    python tools/device_qcoder_ab.py --out profiles/r21_device_qcoder_ab.json
"""
import argparse
import hashlib
import importlib
import json
import os
import resource
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cpu_seconds():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", type=int, default=256)
    ap.add_argument("--small", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--buffers", type=int, nargs="+", default=[0, 128, 1024], help="n_host_buffers values (0: the context's default for the slot count)")
    ap.add_argument("--symbols-per-launch", type=int, default=0)
    ap.add_argument("--sets", nargs="+", default=["small", "big"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("nblic-image-compression_amd")
    dev = torch.device("cuda:0")
    doc = {"what": "effort-0 entropy stage: host coder threads (mode 0), device rANS stage (1), shared (2)", "unit": "Mpixel/s",
           "symbols_per_launch": args.symbols_per_launch, "runs": args.runs, "sets": {}}
    for name in args.sets:
        count, side = (args.big, 4096) if name == "big" else (args.small, 512)
        base = torch.from_numpy(pkg.syn1(side, side, 1)).to(dev)
        frames = [torch.roll(base, shifts=k, dims=1).contiguous() for k in range(min(count, 16))]     # sixteen distinct frames, repeated
        ptrs = [frames[k % len(frames)].data_ptr() for k in range(count)]
        shapes = [(side, side)] * count
        probe = (0, count // 2, count - 1)
        ref = {}
        legs = []
        for run in range(args.runs):
            for mode in (0, 1, 2):                                       # alternating: every run visits every mode
                for nb in args.buffers:
                    slots = min(count, 48)
                    ctx = pkg.Context(device=0, n_slots=slots, n_coders=16, n_groups=6, n_host_buffers=nb or slots + 16 * 16 + 32)
                    try:
                        ctx.set_device_qcoder(mode, args.symbols_per_launch)
                        torch.cuda.synchronize()
                        c0, t0 = cpu_seconds(), time.perf_counter()
                        outs, lens = ctx.qencode_ptrs(ptrs, shapes, True)
                        wall, cpu = time.perf_counter() - t0, cpu_seconds() - c0
                        st = ctx.device_qcoder_stats()
                    finally:
                        ctx.close()
                    digest = [hashlib.sha256(outs[k][:int(lens[k])].tobytes()).hexdigest() for k in probe]
                    if mode == 0:
                        ref.setdefault("digest", digest)
                    leg = {"run": run, "mode": mode, "n_host_buffers": nb, "wall_s": round(wall, 4), "mpixel_per_s": round(count * side * side / wall / 1e6, 1),
                           "cpu_s": round(cpu, 3), "device_images": st["images"], "launches": st["launches"], "kernel_ms": round(st["kernel_ms"], 2),
                           # a launch advances every unfinished lane by the budget: launches x budget / kernel time is one lane's rate
                           "lane_symbols_per_s": round(st["launches"] * (args.symbols_per_launch or 32768) / st["kernel_ms"] * 1e3, 1) if st["kernel_ms"] > 0 else None,
                           "stage_symbols_per_s": round(st["symbols"] / st["kernel_ms"] * 1e3, 1) if st["kernel_ms"] > 0 else None,
                           "streams_equal_mode0": digest == ref["digest"]}
                    legs.append(leg)
                    print(name, json.dumps(leg), flush=True)
                    if args.out:                                         # after every leg: a run that is cut short keeps what it measured
                        doc["sets"][name] = {"frames": count, "side": side, "legs": legs}
                        with open(args.out, "w") as f:
                            json.dump(doc, f, indent=1)
                    del outs
        summary = {}
        for mode in (0, 1, 2):
            for nb in args.buffers:
                v = [l for l in legs if l["mode"] == mode and l["n_host_buffers"] == nb]
                summary[f"mode{mode}_buffers{nb}"] = {"mpixel_per_s_median": statistics.median(l["mpixel_per_s"] for l in v),
                                                     "cpu_s_median": statistics.median(l["cpu_s"] for l in v),
                                                     "all_streams_equal": all(l["streams_equal_mode0"] for l in v)}
        doc["sets"][name] = {"frames": count, "side": side, "legs": legs, "summary": summary}
        if args.out:
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
    print(json.dumps({k: v["summary"] for k, v in doc["sets"].items()}))


if __name__ == "__main__":
    main()
