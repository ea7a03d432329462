"""A/B figures for the per-frame colour plan (Context.color_plan, color=modes), one leg per invocation, merged into --out:

  --leg size
      total stream bytes of 16 frames of 1024 x 1024 per class, at -e1 and at effort 0, coded four ways: plain; the fixed
      transform (color="rct"); planned (color=color_plan(src)); and the per-frame best of all ten modes (exhaustive: every
      frame coded in every mode, the smallest three streams kept).  Classes: shared (the channels share a SYN-1 plane),
      independent (three seeds) -- the two of tools/rct_ab.py -- rb_shared (R and B share a plane, G is independent) and
      mix (all three kinds in one call).  All constructed: no colour photograph was at hand.
  --leg time
      16 frames of 4096 x 4096 as uint8 NHWC and as float16 channels-last: GPU milliseconds of the cost launch
      (nblic_amd_color_plan_stats) next to the collect launches' (nblic_amd_collect_ms) of encoding the same frames with
      the planned modes, and the wall seconds of plan + encode against encode with "rct".  Median of three, min-to-max spread.
  --leg bench --parent-lib PARENT/libnblic_amd.so
      python bench.py with the parent commit's library (through NBLIC_AMD_LIB) and with this tree's, alternating, three
      runs each, every run a process of its own under its own time limit; this tree's median must lie within the parent's
      own min-to-max spread of the parent's median.

On the GPU box, every leg under a limit of its own:
    timeout -k 10 500 python tools/color_plan_ab.py --leg size --out profiles/r26_color_plan_ab.json && \\
    timeout -k 10 500 python tools/color_plan_ab.py --leg time --out profiles/r26_color_plan_ab.json && \\
    timeout -k 10 1100 python tools/color_plan_ab.py --leg bench --parent-lib PARENT/libnblic_amd.so --out profiles/r26_bench_ab.json
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--leg", required=True, choices=("size", "time", "bench"))
ap.add_argument("--out", required=True)
ap.add_argument("--parent-lib", default="")
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--bench-args", default="--gpus 1 --steps 10 --warmup 3")
ap.add_argument("--bench-limit", type=int, default=170, help="seconds one bench.py run may take")
args = ap.parse_args()


def stat(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4),
            "spread": round(max(values) - min(values), 4), "runs": [round(v, 4) for v in values]}


def merge(doc):
    old = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
    old.update(doc)
    with open(args.out, "w") as f:
        json.dump(old, f, indent=1)
        f.write("\n")


def leg_bench():
    assert args.parent_lib, "--leg bench needs --parent-lib"
    runs = {"parent": [], "tree": []}
    lines = {"parent": [], "tree": []}
    for k in range(3):
        for lib in ("parent", "tree"):
            env = dict(os.environ)
            env.pop("NBLIC_AMD_LIB", None)
            if lib == "parent":
                env["NBLIC_AMD_LIB"] = os.path.abspath(args.parent_lib)
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args.bench_args.split(), env=env, capture_output=True, text=True,
                               timeout=args.bench_limit)
            if r.returncode != 0:                               # nothing more is started on the GPU after a run that failed
                print(r.stdout[-2000:], r.stderr[-2000:])
                raise SystemExit(f"bench.py failed with the {lib} library (rc {r.returncode})")
            line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            runs[lib].append(float(line["value"]))
            lines[lib].append({k2: line[k2] for k2 in ("metric", "value", "unit") if k2 in line})
            print(lib, k, line.get("value"), flush=True)
    p, t = stat(runs["parent"]), stat(runs["tree"])
    doc = {"what": "python bench.py " + args.bench_args + ", parent commit's library and this tree's alternating in one GPU call, three runs each",
           "parent": p, "tree": t, "lines": lines,
           "tree_median_minus_parent_median": round(t["median"] - p["median"], 4),
           "tree_slower_than_parent_by": round(max(p["median"] - t["median"], 0.0), 4), "parent_spread": p["spread"],
           "within_parent_spread": bool(p["median"] - t["median"] <= p["spread"])}      # (the value is a rate: higher is faster)
    merge(doc)
    print(json.dumps({k: doc[k] for k in ("parent", "tree", "within_parent_spread")}))


def frame_of(pkg, np, kind, f, h, w):
    """[h, w, 3] uint8.  shared: a SYN-1 plane in every channel plus an eighth of an independent SYN-1 plane (as
    tools/rct_ab.py); independent: three seeds; rb_shared: R and B as in shared, G a seed of its own."""
    out = np.empty((h, w, 3), np.uint8)
    base = pkg.syn1(h, w, 500 + f).astype(np.uint16)
    for c in range(3):
        own = pkg.syn1(h, w, (600 if kind != "independent" else 700) + 3 * f + c)
        mixed = np.clip(base * 7 // 8 + own // 8, 0, 255).astype(np.uint8)
        out[:, :, c] = own if kind == "independent" or (kind == "rb_shared" and c == 1) else mixed
    return out


KINDS = ("shared", "independent", "rb_shared")


def frames_of(pkg, np, kind, n, h, w):
    return np.stack([frame_of(pkg, np, KINDS[f % 3] if kind == "mix" else kind, f, h, w) for f in range(n)])


def leg_size():
    import numpy as np
    import torch
    torch.cuda.init()
    pkg = importlib.import_module("nblic-image-compression_amd")
    ctx = pkg.Context(device=0, n_slots=8, n_coders=8)
    n, h, w = args.frames, 1024, 1024
    doc = {"frames": n, "height": h, "width": w, "raw_bytes": n * 3 * h * w, "classes": {}}
    for kind in KINDS + ("mix",):
        src = torch.from_numpy(frames_of(pkg, np, kind, n, h, w)).cuda().permute(0, 3, 1, 2)
        torch.cuda.synchronize()
        planned, costs = ctx.color_plan(src, costs=True)
        rec = {"planned_modes": ["0x%02x" % m for m in planned], "costs_frame0": [int(v) for v in costs[0]]}
        for effort in (1, 0):
            per_mode = {}
            for m in pkg.COLOR_MODES:                           # every frame in every mode
                got = ctx.encode_batch_from(src, effort=effort, color=[m] * n)
                assert all(s is not None for s in got)
                per_mode[m] = [sum(len(s) for s in got[3 * f:3 * f + 3]) for f in range(n)]
            rct = ctx.encode_batch_from(src, effort=effort, color="rct")
            assert [sum(len(s) for s in rct[3 * f:3 * f + 3]) for f in range(n)] == per_mode[pkg.COLOR_RCT]
            got = ctx.encode_batch_from(src, effort=effort, color=planned)
            plan_bytes = sum(len(s) for s in got)
            assert plan_bytes == sum(per_mode[int(m)][f] for f, m in enumerate(planned))
            plain, fixed = sum(per_mode[0]), sum(per_mode[pkg.COLOR_RCT])
            best_modes = [min(pkg.COLOR_MODES, key=lambda m: per_mode[m][f]) for f in range(n)]
            best = sum(per_mode[m][f] for f, m in enumerate(best_modes))
            rec[f"effort{effort}"] = {"plain_bytes": plain, "rct_bytes": fixed, "planned_bytes": plan_bytes, "exhaustive_bytes": best,
                                      "exhaustive_modes": ["0x%02x" % m for m in best_modes],
                                      "planned_over_plain": round(plan_bytes / plain, 4), "planned_over_rct": round(plan_bytes / fixed, 4),
                                      "planned_over_exhaustive": round(plan_bytes / best, 4), "rct_over_plain": round(fixed / plain, 4),
                                      "planned_no_larger_than_min_of_plain_and_rct": bool(plan_bytes <= min(plain, fixed))}
            print(kind, effort, json.dumps(rec[f"effort{effort}"]), flush=True)
        doc["classes"][kind] = rec
    ctx.close()
    merge({"size": doc})


def leg_time():
    import numpy as np
    import torch
    torch.cuda.init()
    pkg = importlib.import_module("nblic-image-compression_amd")
    ctx = pkg.Context(device=0, n_slots=12, n_coders=12)
    n, h, w = args.frames, 4096, 4096
    small = frames_of(pkg, np, "mix", 4, 1024, 1024)
    host = np.tile(small, (n // 4, 4, 4, 1))                    # 16 frames of 4096 x 4096: the content is not what is timed
    ctx.enable_timing(True)
    doc = {"frames": n, "height": h, "width": w}
    for name in ("uint8_nhwc", "float16_channels_last"):
        if name == "uint8_nhwc":
            src, scale = torch.from_numpy(host).cuda().permute(0, 3, 1, 2), 1.0
        else:
            src = torch.from_numpy(host).cuda().permute(0, 3, 1, 2).to(torch.float16).div_(255.0).contiguous(memory_format=torch.channels_last)
            scale = 255.0
        torch.cuda.synchronize()
        modes = ctx.color_plan(src, scale=scale)                # (warm-up)
        assert all(s is not None for s in ctx.encode_batch_from(src, scale=scale, color=modes))
        assert all(s is not None for s in ctx.encode_batch_from(src, scale=scale, color="rct"))
        cost_ms, plan_wall, collect, planned_wall, rct_wall = [], [], [], [], []
        for _ in range(3):
            t0 = time.perf_counter()
            modes = ctx.color_plan(src, scale=scale)
            t1 = time.perf_counter()
            ms0, k0 = ctx.collect_ms()
            got = ctx.encode_batch_from(src, scale=scale, color=modes)
            t2 = time.perf_counter()
            ms1, k1 = ctx.collect_ms()
            assert all(s is not None for s in got)
            cost_ms.append(ctx.color_plan_stats()[2]); plan_wall.append(t1 - t0); planned_wall.append(t2 - t0); collect.append(ms1 - ms0)
            t0 = time.perf_counter()
            got = ctx.encode_batch_from(src, scale=scale, color="rct")
            rct_wall.append(time.perf_counter() - t0)
            assert all(s is not None for s in got)
        doc[name] = {"planned_modes": ["0x%02x" % m for m in modes], "cost_launch_gpu_ms": stat(cost_ms), "color_plan_wall_s": stat(plan_wall),
                     "collect_gpu_ms_of_the_planned_encode": stat(collect), "collect_launches_timed_last": k1 - k0,
                     "plan_plus_encode_wall_s": stat(planned_wall), "encode_rct_wall_s": stat(rct_wall)}
        print(name, json.dumps(doc[name]), flush=True)
        del src
    ctx.close()
    merge({"time": doc})


if args.leg == "bench":
    leg_bench()
elif args.leg == "time":
    leg_time()
else:
    leg_size()
