"""A/B figures for the reversible colour transform (color="rct"), one leg per invocation, merged into --out:

  --leg size_shared | size_independent
      bytes of the three streams of 16 frames of 1024 x 1024 with and without the flag, at -e1 and at effort 0.  shared: the
      channels share a SYN-1 plane and differ by small independent SYN-1 chroma; independent: three unrelated seeds, where
      the transform must lose.  Both classes are constructed: no colour photograph was at hand.
  --leg time
      encode_batch_from and decode_batch_indexed_into on 48 planes of 4096 x 4096 laid out as 16 NHWC frames, with and
      without the flag: wall seconds, the collect launches' GPU milliseconds (nblic_amd_collect_ms) and the delivery's
      milliseconds (nblic_amd_indexed_decode_split, the last part).  Median of three, min-to-max spread.
  --leg bench --parent-lib PARENT/libnblic_amd.so
      python bench.py with the parent commit's library (through NBLIC_AMD_LIB) and with this tree's, alternating, three
      runs each, every run a process of its own under its own time limit; this tree's median must lie within the parent's
      own min-to-max spread of the parent's median.

On the GPU box, every leg under a limit of its own:
    timeout -k 10 300 python tools/rct_ab.py --leg size_shared --out profiles/r25_rct_ab.json && \\
    timeout -k 10 300 python tools/rct_ab.py --leg size_independent --out profiles/r25_rct_ab.json && \\
    timeout -k 10 600 python tools/rct_ab.py --leg time --out profiles/r25_rct_ab.json && \\
    timeout -k 10 1100 python tools/rct_ab.py --leg bench --parent-lib PARENT/libnblic_amd.so --out profiles/r25_bench_ab.json
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
ap.add_argument("--leg", required=True, choices=("size_shared", "size_independent", "time", "bench"))
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


def frames_of(pkg, np, kind, n, h, w):
    """[n, h, w, 3] uint8.  shared: a SYN-1 plane in every channel plus an eighth of an independent SYN-1 plane;
    independent: three seeds."""
    out = np.empty((n, h, w, 3), np.uint8)
    for f in range(n):
        if kind == "shared":
            base = pkg.syn1(h, w, 500 + f).astype(np.uint16)
            for c in range(3):
                out[f, :, :, c] = np.clip(base * 7 // 8 + pkg.syn1(h, w, 600 + 3 * f + c) // 8, 0, 255).astype(np.uint8)
        else:
            for c in range(3):
                out[f, :, :, c] = pkg.syn1(h, w, 700 + 3 * f + c)
    return out


def leg_size(kind):
    import numpy as np
    import torch
    torch.cuda.init()
    pkg = importlib.import_module("nblic-image-compression_amd")
    ctx = pkg.Context(device=0, n_slots=8, n_coders=8)
    n, h, w = args.frames, 1024, 1024
    src = torch.from_numpy(frames_of(pkg, np, kind, n, h, w)).cuda().permute(0, 3, 1, 2)
    torch.cuda.synchronize()
    doc = {"frames": n, "height": h, "width": w, "raw_bytes": n * 3 * h * w}
    for effort in (1, 0):
        plain = ctx.encode_batch_from(src, effort=effort)
        rct = ctx.encode_batch_from(src, effort=effort, color="rct")
        assert all(s is not None for s in plain + rct)
        a, b = sum(len(s) for s in plain), sum(len(s) for s in rct)
        per = lambda ss: [sum(len(s) for s in ss[c::3]) for c in range(3)]
        doc[f"effort{effort}"] = {"plain_bytes": a, "rct_bytes": b, "rct_over_plain": round(b / a, 4), "plain_per_channel": per(plain), "rct_per_channel": per(rct)}
        print(kind, effort, a, b, round(b / a, 4), flush=True)
    ctx.close()
    merge({f"size_{kind}": doc})


def leg_time():
    import numpy as np
    import torch
    torch.cuda.init()
    pkg = importlib.import_module("nblic-image-compression_amd")
    ctx = pkg.Context(device=0, n_slots=12, n_coders=12)
    n, h, w = args.frames, 4096, 4096
    small = frames_of(pkg, np, "shared", 2, 1024, 1024)
    host = np.tile(small, (n // 2, 4, 4, 1))                    # 16 frames of 4096 x 4096: the content is not what is timed
    src = torch.from_numpy(host).cuda().permute(0, 3, 1, 2)
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda").permute(0, 3, 1, 2)
    torch.cuda.synchronize()
    ctx.enable_timing(True)
    doc = {"planes": 3 * n, "height": h, "width": w}
    for name, color in (("plain", None), ("rct", "color")):
        kw = {"color": "rct"} if color else {}
        pairs = ctx.encode_batch_from(src, every_rows=256, **kw)      # (warm-up, and the indexed pairs the decode takes)
        assert all(s is not None and x is not None for s, x in pairs)
        enc_wall, collect, dec_wall, deliver = [], [], [], []
        for _ in range(3):
            ms0, k0 = ctx.collect_ms()
            t0 = time.perf_counter()
            got = ctx.encode_batch_from(src, **kw)
            enc_wall.append(time.perf_counter() - t0)
            ms1, k1 = ctx.collect_ms()
            collect.append(ms1 - ms0)
            assert all(s is not None for s in got)
        assert ctx.decode_batch_indexed_into(pairs, out, layout="any", **kw) == [0] * (3 * n)
        for _ in range(3):
            t0 = time.perf_counter()
            status = ctx.decode_batch_indexed_into(pairs, out, layout="any", **kw)
            dec_wall.append(time.perf_counter() - t0)
            deliver.append(ctx.indexed_decode_split()["copy_out"])
            assert status == [0] * (3 * n)
        if color:
            torch.cuda.synchronize()
            assert bool((out == src).all()), "the decoded frames differ from the sources"
        doc[name] = {"encode_wall_s": stat(enc_wall), "collect_gpu_ms": stat(collect), "collect_launches_timed_last": k1 - k0,
                     "decode_wall_s": stat(dec_wall), "delivery_ms": stat(deliver)}
        print(name, json.dumps(doc[name]), flush=True)
    ctx.close()
    merge({"time": doc})


if args.leg == "bench":
    leg_bench()
elif args.leg == "time":
    leg_time()
else:
    leg_size(args.leg.split("_")[1])
