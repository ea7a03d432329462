"""Same-box A/B of two ways to get a batch of indexed streams into a batch tensor on the GPU, in one process on one GPU:

  a        what a caller does without the delivery: Context.decode_batch_indexed to numpy, np.stack, one copy to the device
           tensor with torch (whole planes, uint8);
  b        Context.decode_batch_indexed_into the same uint8 tensor, whole planes;
  a_crop   as a, with the caller's crop and normalisation on the host in front of the upload: columns [COL0, COL0 + 224) of
           every plane, float32(px) * (1 / 255), converted to float16;
  c        Context.decode_batch_indexed_into a float16 tensor with scale = 1 / 255 and the same 224-column window.

The batch tensors are allocated once, outside the timed region (a loader reuses them).  Every leg of every run gets a FRESH
context (made and closed outside the timed region); one warm-up per leg, then --repeat runs per leg, alternating; wall time
per run, medians with min-to-max spreads; every tensor of every run is compared with the inputs (c and a_crop with the numpy
expression, bit for bit).  Every run records Context.indexed_decode_split (host checks, uploads, rounds, copy-out -- for b
and c the copy-out is the delivery launch).  Three settings, those of profiles/r14_indexed_batch_decode_ab.json:

  large    16 SYN-1 frames of 4096 x 4096 at R = 64;
  small    64 frames of 1024 x 1024 at R = 32;
  rows     rows [300, 500) of each of those 64.

Each setting is one process; run each under its own time limit and chain them, so that a fault ends the sequence:

    timeout -k 10 900 python tools/decode_to_device_ab.py --setting large --out profiles/r22_decode_to_device_ab.json && \\
    timeout -k 10 600 python tools/decode_to_device_ab.py --setting small --out profiles/r22_decode_to_device_ab.json && \\
    timeout -k 10 600 python tools/decode_to_device_ab.py --setting rows --out profiles/r22_decode_to_device_ab.json

A setting's result is merged into --out under its name.
"""
import argparse, importlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--setting", choices=("large", "small", "rows", "quick"), default="large")
ap.add_argument("--repeat", type=int, default=3)
args = ap.parse_args()

torch.cuda.init()                                       # (torch first: the library binds to the HIP runtime that is already loaded)
pkg = importlib.import_module("nblic-image-compression_amd")
N, H, W, R, ROWS = {"large": (16, 4096, 4096, 64, None), "small": (64, 1024, 1024, 32, None), "rows": (64, 1024, 1024, 32, (300, 500)),
                    "quick": (6, 256, 256, 16, (80, 130))}[args.setting]
COLS = ((W - 224) // 2 + 1, (W - 224) // 2 + 225)       # an odd first column
SCALE = 1.0 / 255.0
R0, R1 = ROWS if ROWS else (0, H)


def context():
    return pkg.Context(device=0, n_slots=48, n_coders=16, n_groups=6)


imgs = [pkg.syn1(H, W, 1 + k) for k in range(N)]
ctx = context()
pairs = ctx.encode_batch_indexed(imgs, R)
ctx.close()
assert all(ix is not None for _, ix in pairs)
rows_arg = [ROWS] * N if ROWS else None
want_u8 = np.stack([i[R0:R1] for i in imgs])
want_f16 = (want_u8[:, :, COLS[0]:COLS[1]].astype(np.float32) * np.float32(SCALE)).astype(np.float16)
out_u8 = torch.empty((N, R1 - R0, W), dtype=torch.uint8, device="cuda")
out_f16 = torch.empty((N, R1 - R0, 224), dtype=torch.float16, device="cuda")


def leg_a(ctx):
    planes = ctx.decode_batch_indexed(pairs, rows_arg)
    out_u8.copy_(torch.from_numpy(np.stack(planes)))
    torch.cuda.synchronize()
    return out_u8


def leg_b(ctx):
    assert ctx.decode_batch_indexed_into(pairs, out_u8, rows=ROWS) == [0] * N
    return out_u8


def leg_a_crop(ctx):
    planes = ctx.decode_batch_indexed(pairs, rows_arg)
    crop = np.stack([p[:, COLS[0]:COLS[1]] for p in planes])
    out_f16.copy_(torch.from_numpy((crop.astype(np.float32) * np.float32(SCALE)).astype(np.float16)))
    torch.cuda.synchronize()
    return out_f16


def leg_c(ctx):
    assert ctx.decode_batch_indexed_into(pairs, out_f16, rows=ROWS, cols=COLS, scale=SCALE) == [0] * N
    return out_f16


legs = {"a": leg_a, "b": leg_b, "a_crop": leg_a_crop, "c": leg_c}


def run(name):
    ctx = context()
    try:
        for t in (out_u8, out_f16):
            t.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = legs[name](ctx)
        wall = time.perf_counter() - t0
        split = ctx.indexed_decode_split()
    finally:
        ctx.close()
    got = res.cpu().numpy()
    want = want_u8 if res is out_u8 else want_f16
    assert got.shape == want.shape and (got.view(np.uint8) == want.view(np.uint8)).all(), name       # bit for bit
    rec = {"leg": name, "wall_s": round(wall, 4), "split_ms": {k: round(v, 2) for k, v in split.items()}}
    print(json.dumps(rec), flush=True)
    return rec


def summarise(runs):
    out = {}
    for name in legs:
        t = [r["wall_s"] for r in runs if r["leg"] == name]
        out[name] = {"runs_s": t, "median_s": round(statistics.median(t), 4), "min_s": min(t), "max_s": max(t), "spread_s": round(max(t) - min(t), 4),
                     "split_ms_median": {k: round(statistics.median(r["split_ms"][k] for r in runs if r["leg"] == name), 2) for k in runs[0]["split_ms"]}}
    return out


def verdict(summary, old, new):
    gain = summary[old]["median_s"] - summary[new]["median_s"]
    return {"old": old, "new": new, "ratio_of_medians": round(summary[old]["median_s"] / summary[new]["median_s"], 3), "gain_s": round(gain, 4),
            "spread_of_old_s": summary[old]["spread_s"], "gain_exceeds_spread": bool(gain > summary[old]["spread_s"]),
            "not_slower_by_more_than_spread": bool(-gain <= summary[old]["spread_s"])}


warm = [run(name) for name in legs]
runs = [run(name) for _ in range(args.repeat) for name in legs]
summary = summarise(runs)
doc = {"what": "indexed streams into a batch tensor on the GPU: decode_batch_indexed to numpy, np.stack and one torch copy to the device (a; a_crop with "
               "the 224-column crop and the float16 normalisation on the host in front of it) against decode_batch_indexed_into (b uint8 whole rows; c "
               "float16, scale 1/255, the 224-column window); streams and indexes from encode_batch_indexed on SYN-1 frames, seeds 1..N; same box, same "
               "process, a fresh context of 6 groups x 8 slots and 16 coder threads per leg and run; batch tensors allocated once; one warm-up per leg, "
               "then the runs alternating; every tensor compared with its input bit for bit",
       "frames": N, "h": H, "w": W, "every_rows": R, "rows": [R0, R1], "cols_of_the_crop": list(COLS), "scale": SCALE,
       "host_bytes_a_keeps_for_planes": int(want_u8.nbytes), "host_bytes_b_keeps_for_planes": 0,
       "warm_up": warm, "runs": runs, "summary": summary, "b_against_a": verdict(summary, "a", "b"), "c_against_a_crop": verdict(summary, "a_crop", "c")}
print(json.dumps({k: v for k, v in doc.items() if "against" in k}), flush=True)
if args.out:
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.load(f)
    merged[args.setting] = doc
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")
