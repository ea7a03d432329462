"""A/B figures for slice stacks (Context.stack_plan, stack=modes), one leg per invocation, merged into --out:

  --leg size
      total stream bytes of 4 stacks of 16 slices of 1024 x 1024 per class, at -e1 and at effort 0, coded four ways: all
      keys; "delta"; planned (stack=stack_plan(src)); and the per-slice best of the two encodes (the choices of a stack's
      slices are independent of each other, so the exhaustive best is the smaller of each slice's two streams).  Classes:
      static (the slices share a SYN-1 plane, 7 parts in 8), independent (a seed per slice), cut (static with another shared
      plane from slice 8 on), equal.  Conditions: planned == keys on the independent class, planned <= "delta" on the cut
      class.  All constructed: no real volume or sequence was at hand.
  --leg time
      64 slices of 4096 x 4096 as uint8 and as float16: GPU milliseconds of the k_stack_cost launch next to the k_collect
      launches of encoding the same slices as deltas; and GPU milliseconds of the delivery launches of decoding 4 runs of
      16 planes into a uint8 and a float16 tensor (k_deliver_stack) next to the same 64 planes delivered plain (k_deliver:
      the same call with every mode 0).  Median of three, min-to-max spread.  Reported, not gated.
  --leg bench --parent-lib PARENT/libnblic_amd.so
      python bench.py with the parent commit's library (through NBLIC_AMD_LIB) and with this tree's, alternating, three
      runs each, every run a process of its own under its own time limit; this tree's median must lie within the parent's
      own min-to-max spread of the parent's median.

On the GPU box, every leg under a limit of its own:
    timeout -k 10 500 python tools/stack_ab.py --leg size --out profiles/r27_stack_ab.json && \\
    timeout -k 10 500 python tools/stack_ab.py --leg time --out profiles/r27_stack_ab.json && \\
    timeout -k 10 1100 python tools/stack_ab.py --leg bench --parent-lib PARENT/libnblic_amd.so --out profiles/r27_bench_ab.json
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--leg", required=True, choices=("size", "time", "bench"))
ap.add_argument("--out", required=True)
ap.add_argument("--parent-lib", default="")
ap.add_argument("--stacks", type=int, default=4)
ap.add_argument("--depth", type=int, default=16)
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


KINDS = ("static", "independent", "cut", "equal")


def stack_of(pkg, np, kind, s, depth, h, w):
    """[depth, h, w] uint8.  static: a SYN-1 plane in every slice plus an eighth of a plane of the slice's own seed; cut: the
    same with another shared plane from slice depth / 2 on; independent: a seed per slice; equal: one plane."""
    mix = lambda a, b: ((7 * a.astype(np.uint16) + b) // 8).astype(np.uint8)
    base, other = pkg.syn1(h, w, 800 + 3 * s), pkg.syn1(h, w, 801 + 3 * s)
    out = np.empty((depth, h, w), np.uint8)
    for d in range(depth):
        own = pkg.syn1(h, w, 900 + 64 * s + d)
        out[d] = own if kind == "independent" else (base if kind == "equal" else mix(other if kind == "cut" and d >= depth // 2 else base, own))
    return out


def leg_size():
    import numpy as np
    import torch
    torch.cuda.init()
    pkg = importlib.import_module("nblic-image-compression_amd")
    ctx = pkg.Context(device=0, n_slots=8, n_coders=8)
    n, depth, h, w = args.stacks, args.depth, 1024, 1024
    doc = {"stacks": n, "depth": depth, "height": h, "width": w, "raw_bytes": n * depth * h * w, "classes": {}}
    for kind in KINDS:
        src = torch.from_numpy(np.stack([stack_of(pkg, np, kind, s, depth, h, w) for s in range(n)])).cuda()
        torch.cuda.synchronize()
        planned, costs = ctx.stack_plan(src, costs=True)
        rec = {"planned_modes_stack0": [int(m) for m in planned[:depth]], "deltas_planned": int(planned.sum()),
               "delta_over_intra_cost_stack0": [round(float(c[1]) / float(c[0]), 4) for c in costs[1:depth]]}
        for effort in (1, 0):
            size = lambda stack: [len(s) for s in ctx.encode_batch_from(src, effort=effort, stack=stack)]
            keys, delta, plan = size([0] * (n * depth)), size("delta"), size(planned)
            best = sum(min(a, b) for a, b in zip(keys, delta))
            assert sum(plan) == sum(d if m else k for k, d, m in zip(keys, delta, planned))      # (the choices are independent of each other)
            rec[f"effort{effort}"] = {"keys_bytes": sum(keys), "delta_bytes": sum(delta), "planned_bytes": sum(plan), "best_bytes": best,
                                      "delta_over_keys": round(sum(delta) / sum(keys), 4), "planned_over_keys": round(sum(plan) / sum(keys), 4),
                                      "best_over_keys": round(best / sum(keys), 4), "planned_over_best": round(sum(plan) / best, 4)}
            print(kind, effort, json.dumps(rec[f"effort{effort}"]), flush=True)
        doc["classes"][kind] = rec
    ctx.close()
    ind, cut = doc["classes"]["independent"], doc["classes"]["cut"]
    doc["conditions"] = {"independent_planned_equals_keys": all(ind[f"effort{e}"]["planned_bytes"] == ind[f"effort{e}"]["keys_bytes"] for e in (0, 1)) and ind["deltas_planned"] == 0,
                         "cut_planned_no_larger_than_delta": all(cut[f"effort{e}"]["planned_bytes"] <= cut[f"effort{e}"]["delta_bytes"] for e in (0, 1))}
    merge({"size": doc})
    print(json.dumps(doc["conditions"]))
    assert all(doc["conditions"].values())


def leg_time():
    import numpy as np
    import torch
    torch.cuda.init()
    pkg = importlib.import_module("nblic-image-compression_amd")
    ctx = pkg.Context(device=0, n_slots=12, n_coders=12)
    n, depth, h, w = args.stacks, args.depth, 4096, 4096
    small = np.stack([stack_of(pkg, np, KINDS[s % 2], s, depth, 512, 512) for s in range(n)])
    host = np.tile(small, (1, 1, 8, 8))                         # 64 slices of 4096 x 4096: the content is not what is timed
    ctx.enable_timing(True)
    doc = {"stacks": n, "depth": depth, "height": h, "width": w}
    for name in ("uint8", "float16"):
        src, scale = torch.from_numpy(host).cuda(), 1.0
        if name == "float16":
            src, scale = src.to(torch.float16).div_(255.0), 255.0
        torch.cuda.synchronize()
        ctx.stack_plan(src, scale=scale)                        # (warm-up)
        cost_ms, collect = [], []
        for _ in range(3):
            ctx.stack_plan(src, scale=scale)
            cost_ms.append(ctx.stack_plan_stats()["plan_ms"])
            ms0, k0 = ctx.collect_ms()
            pairs = ctx.encode_batch_from(src, scale=scale, effort=0, every_rows=64, stack="delta")      # (with indexes: the decodes below run their segments side by side)
            ms1, k1 = ctx.collect_ms()
            assert all(s is not None and x is not None for s, x in pairs)
            collect.append(ms1 - ms0)
        doc["cost_" + name] = {"k_stack_cost_gpu_ms": stat(cost_ms), "k_collect_gpu_ms_of_the_delta_encode": stat(collect), "collect_launches_timed_last": k1 - k0}
        print(name, json.dumps(doc["cost_" + name]), flush=True)
        del src
        out = torch.empty((n, depth, h, w), dtype=getattr(torch, name), device="cuda")
        fscale = 1.0 if name == "uint8" else 1.0 / 255.0
        runs, plain = [], []
        for k in range(4):                                      # (the first round is the warm-up)
            assert ctx.decode_batch_indexed_into(pairs, out, stack="delta", scale=fscale) == [0] * (n * depth)
            a = ctx.stack_plan_stats()["deliver_ms"]
            if k == 3:
                torch.cuda.synchronize()
                assert np.array_equal(out[n - 1, depth - 1].cpu().numpy().view(np.uint8), (host[n - 1, depth - 1] if name == "uint8" else
                                      (host[n - 1, depth - 1].astype(np.float32) * np.float32(fscale)).astype(np.float16)).view(np.uint8))
            assert ctx.decode_batch_indexed_into(pairs, out, stack=[0] * (n * depth), depth=depth, scale=fscale) == [0] * (n * depth)
            b = ctx.stack_plan_stats()["deliver_ms"]
            if k:
                runs.append(a); plain.append(b)
        doc["deliver_" + name] = {"k_deliver_stack_gpu_ms_4_runs_of_16": stat(runs), "k_deliver_gpu_ms_64_planes_plain": stat(plain)}
        print(name, json.dumps(doc["deliver_" + name]), flush=True)
        del out
    ctx.close()
    merge({"time": doc})


if args.leg == "bench":
    leg_bench()
elif args.leg == "time":
    leg_time()
else:
    leg_size()
