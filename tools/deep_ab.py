"""A/B figures for deep pixels (Context.deep_plan, deep=modes), one leg per invocation, merged into --out:

  --leg size
      total stream bytes of --images deep images of 1024 x 1024 per class, at -e1 and at effort 0, coded three ways:
      deep="plain" -- what a caller could do before, with a torch byte split and the existing call; the bytes are verified
      equal once -- deep="fold" and deep="plan".  Classes: tests/deep_inputs.py's, the uniform 16-bit noise among them.
      Condition: planned <= min(plain, fold) on every line; a miss is reported with its size, not tuned away.  All
      constructed: no real radiograph or CT slice was at hand.
  --leg time
      --images deep images of 4096 x 4096 (uint16): GPU milliseconds of the k_collect_deep launch next to the torch split
      (x >> 8, x & 255, .to(uint8); torch events) that feeds the existing in-place path, with the split's temporaries in bytes;
      of the k_deliver_deep launch into uint16 and into float16 next to the torch join of two delivered planes; of the
      k_deep_cost launch next to the collect launch of encoding the same images; and the wall time of plan + encode and of
      decode by either route, alternating.  Median of three, min-to-max spread.  Reported, not gated.  Strided
      destinations and the existing route's own k_deliver launches are not timed.
  --leg bench --parent-lib PARENT/libnblic_amd.so
      python bench.py with the parent commit's library (through NBLIC_AMD_LIB) and with this tree's, alternating, three
      runs each, every run a process of its own under its own time limit; this tree's median must lie within the parent's
      own min-to-max spread of the parent's median.

On the GPU box, every leg under a limit of its own:
    timeout -k 10 500 python tools/deep_ab.py --leg size --out profiles/r28_deep_ab.json && \\
    timeout -k 10 500 python tools/deep_ab.py --leg time --out profiles/r28_deep_ab.json && \\
    timeout -k 10 1100 python tools/deep_ab.py --leg bench --parent-lib PARENT/libnblic_amd.so --out profiles/r28_bench_ab.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--leg", required=True, choices=("size", "time", "bench"))
ap.add_argument("--out", required=True)
ap.add_argument("--parent-lib", default="")
ap.add_argument("--images", type=int, default=16)
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


def split(torch, x):
    """What a caller had to do before: two uint8 planes per image, by torch.  x: [n, h, w] int32 copies of the 16-bit values
    would double the traffic, so the shifts run on the int16 view, whose bits they are."""
    v = x.view(torch.int16)
    return torch.stack((((v >> 8) & 255).to(torch.uint8), (v & 255).to(torch.uint8)), dim=1)


def leg_size():
    import numpy as np
    import torch
    import deep_inputs as di
    torch.cuda.init()
    pkg = importlib.import_module("nblic-image-compression_amd")
    ctx = pkg.Context(device=0, n_slots=8, n_coders=8)
    n, h, w = args.images, 1024, 1024
    doc = {"images": n, "height": h, "width": w, "raw_bytes_per_class": 2 * n * h * w, "classes": {}, "misses": []}
    checked = False
    for name in list(di.CLASSES) + list(di.UNPLANNED):
        host = np.stack([di.class_image(name, h, w, seed=s, syn1=pkg.syn1) for s in range(n)])
        src = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        modes, costs, ranges = ctx.deep_plan(src, costs=True)
        rec = {"folds_planned": int((modes & 1).sum()), "fold_over_plain_cost_image0": round(float(costs[0][2]) / float(costs[0][1]), 4),
               "range": [int(ranges[:, 0].min()), int(ranges[:, 1].max())]}
        for effort in (1, 0):
            size = lambda deep: [len(s) for s in ctx.encode_batch_from(src, effort=effort, deep=deep)]
            plain, fold, plan = size("plain"), size("fold"), size(modes)
            if not checked:                                     # once: "plain" IS the torch byte split through the existing call
                planes = split(torch, src).reshape(2 * n, h, w).contiguous()
                torch.cuda.synchronize()
                assert [len(s) for s in ctx.encode_batch_from(planes, effort=effort)] == plain and ctx.encode_batch_from(planes, effort=effort) == ctx.encode_batch_from(src, effort=effort, deep="plain")
                checked = True
                doc["plain_equals_the_torch_split_through_the_existing_call"] = True
            best = min(sum(plain), sum(fold))
            rec[f"effort{effort}"] = {"plain_bytes": sum(plain), "fold_bytes": sum(fold), "planned_bytes": sum(plan), "fold_over_plain": round(sum(fold) / sum(plain), 4),
                                      "planned_over_plain": round(sum(plan) / sum(plain), 4), "planned_minus_min_plain_fold": sum(plan) - best}
            if sum(plan) > best:
                doc["misses"].append({"class": name, "effort": effort, "bytes_over": sum(plan) - best, "relative": round((sum(plan) - best) / best, 6)})
            print(name, effort, json.dumps(rec[f"effort{effort}"]), flush=True)
        doc["classes"][name] = rec
    ctx.close()
    doc["planned_no_larger_than_min_of_plain_and_fold_on_every_line"] = not doc["misses"]
    merge({"size": doc})
    print(json.dumps({"misses": doc["misses"]}))


def leg_time():
    import numpy as np
    import torch
    import deep_inputs as di
    torch.cuda.init()
    pkg = importlib.import_module("nblic-image-compression_amd")
    ctx = pkg.Context(device=0, n_slots=12, n_coders=12)
    n, h, w = args.images, 4096, 4096
    small = np.stack([di.class_image(list(di.CLASSES)[s % 5], 512, 512, seed=s, syn1=pkg.syn1) for s in range(n)])
    host = np.tile(small, (1, 8, 8))                            # the content is not what is timed
    src = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    doc = {"images": n, "height": h, "width": w, "source_bytes": int(host.nbytes)}

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = fn(); b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b), out

    modes = ctx.deep_plan(src)                                   # (warm-up)
    split(torch, src)
    cost_ms, collect_ms, split_ms, wall_deep, wall_split = [], [], [], [], []
    streams = None
    for _ in range(3):
        t0 = time.perf_counter()
        modes = ctx.deep_plan(src)
        streams = ctx.encode_batch_from(src, effort=0, deep=modes, every_rows=64)      # (with indexes: the decodes below run their segments side by side)
        wall_deep.append((time.perf_counter() - t0) * 1e3)
        s = ctx.deep_plan_stats()
        cost_ms.append(s["plan_ms"]); collect_ms.append(s["collect_ms"])
        assert all(x is not None and i is not None for x, i in streams)
        t0 = time.perf_counter()
        ms, planes = events(lambda: split(torch, src).reshape(2 * n, h, w))
        old = ctx.encode_batch_from(planes, effort=0, every_rows=64)
        wall_split.append((time.perf_counter() - t0) * 1e3)
        split_ms.append(ms)
        del planes
    doc["collect"] = {"k_collect_deep_gpu_ms": stat(collect_ms), "torch_split_gpu_ms": stat(split_ms), "k_deep_cost_gpu_ms": stat(cost_ms),
                      "torch_split_temporaries_bytes": int(host.nbytes) * 2 + int(host.nbytes),      # two int16 intermediates per plane as they live, and the stacked planes
                      "wall_ms_plan_and_indexed_encode_effort0": stat(wall_deep), "wall_ms_torch_split_and_indexed_encode_effort0_plain_only": stat(wall_split)}
    print(json.dumps(doc["collect"]), flush=True)
    plain_streams = old
    for name in ("uint16", "float16"):
        out = torch.empty((n, h, w), dtype=getattr(torch, name), device="cuda")
        planes = torch.empty((2 * n, h, w), dtype=torch.uint8, device="cuda")
        deliver_ms, join_ms, wall_d, wall_j = [], [], [], []
        for k in range(4):                                      # (the first round is the warm-up)
            t0 = time.perf_counter()
            assert ctx.decode_batch_indexed_into(streams, out, deep=modes, scale=1.0 if name == "uint16" else 1.0 / 16.0) == [0] * (2 * n)
            a = (time.perf_counter() - t0) * 1e3
            d = ctx.deep_plan_stats()["deliver_ms"]
            if k == 3 and name == "uint16":
                torch.cuda.synchronize()
                assert np.array_equal(out[n - 1].cpu().numpy(), host[n - 1])
            t0 = time.perf_counter()
            assert ctx.decode_batch_indexed_into(plain_streams, planes) == [0] * (2 * n)
            p = planes.view(n, 2, h, w)
            if name == "uint16":
                ms, _ = events(lambda: ((p[:, 0].to(torch.int32) << 8) | p[:, 1].to(torch.int32)).to(torch.int16).view(torch.uint16))
            else:
                ms, _ = events(lambda: ((p[:, 0].to(torch.float32) * 256.0 + p[:, 1].to(torch.float32)) * (1.0 / 16.0)).to(torch.float16))
            b = (time.perf_counter() - t0) * 1e3
            if k:
                deliver_ms.append(d); join_ms.append(ms); wall_d.append(a); wall_j.append(b)
        doc["deliver_" + name] = {"k_deliver_deep_gpu_ms": stat(deliver_ms), "torch_join_gpu_ms_without_the_planes_delivery": stat(join_ms),
                                  "wall_ms_decode_deep": stat(wall_d), "wall_ms_decode_planes_and_torch_join": stat(wall_j)}
        print(name, json.dumps(doc["deliver_" + name]), flush=True)
        del out, planes
    doc["not_timed"] = ["strided destinations", "the existing route's own k_deliver launches (the library does not report them)"]
    ctx.close()
    merge({"time": doc})


if args.leg == "bench":
    leg_bench()
elif args.leg == "time":
    leg_time()
else:
    leg_size()
