"""Same-box A/B of three ways to read a batch of indexed streams back, in one process on one GPU:

  a        Context.decode_indexed for each image in turn;
  a_thr    one thread per image (at most 16 at a time), one decode_indexed call each;
  b        one Context.decode_batch_indexed call.

decode_indexed and decode_rows are decode_batch_indexed with one image, so a, a_thr and rows_a measure what a call of
that path costs per image against one call for all of them.  (In profiles/r14_indexed_batch_decode_ab.json, and with an
older library behind NBLIC_AMD_LIB, they measure the single calls' former host-side path.)

Streams and indexes come from Context.encode_batch_indexed.  One warm-up per leg, then --repeat runs per leg, alternating;
wall time per run; every plane of every run is compared with its input.  Leg b also reports where the call spent its time
(Context.indexed_decode_split: host checks, uploads, rounds, copy-out).  Two settings:

  large    16 SYN-1 frames of 4096 x 4096 at R = 64 (1024 segments);
  small    64 frames of 1024 x 1024 at R = 32 (2048 segments: the decoders' lean image), and rows [300, 500) of every frame
           through decode_rows in a loop (rows_a) against one decode_batch_indexed call (rows_b).

Each setting is one process; run each under its own time limit and chain them, so that a fault ends the sequence:

    timeout -k 10 900 python tools/indexed_batch_decode_ab.py --setting large --out profiles/r14_indexed_batch_decode_ab.json && \\
    timeout -k 10 600 python tools/indexed_batch_decode_ab.py --setting small --out profiles/r14_indexed_batch_decode_ab.json

A setting's result is merged into --out under its name.  --bench NAME=FILE ... merges the JSON lines of bench.py runs
(one file per library) into the same document and exits.
"""
import argparse, importlib, json, os, statistics, sys, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--setting", choices=("large", "small", "quick"), default="large")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--bench", nargs="*", default=None)
args = ap.parse_args()


def merge(key, value):
    doc = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc[key] = value
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def summarise(runs, names, pixels):
    out = {}
    for name in names:
        t = [r["wall_s"] for r in runs if r["leg"] == name]
        out[name] = {"runs_s": t, "median_s": round(statistics.median(t), 4), "min_s": min(t), "max_s": max(t), "spread_s": round(max(t) - min(t), 4),
                     "median_mpixel_per_s": round(pixels / statistics.median(t) / 1e6, 1)}
    return out


def verdict(summary, old, new):
    gain = summary[old]["median_s"] - summary[new]["median_s"]
    return {"old": old, "new": new, "ratio_of_medians": round(summary[old]["median_s"] / summary[new]["median_s"], 2), "gain_s": round(gain, 4),
            "spread_of_old_s": summary[old]["spread_s"], "gain_exceeds_spread": bool(gain > summary[old]["spread_s"])}


if args.bench is not None:
    lines = {}
    for item in args.bench:
        name, _, path = item.partition("=")
        with open(path) as f:
            lines[name] = [json.loads(l) for l in f if l.strip().startswith("{")]
    merge("bench", lines)
    sys.exit(0)

pkg = importlib.import_module("nblic-image-compression_amd")
N, H, W, R = {"large": (16, 4096, 4096, 64), "small": (64, 1024, 1024, 32), "quick": (6, 256, 256, 16)}[args.setting]
ROWS = (300, 500) if H > 500 else (H // 3, H // 2)
ctx = pkg.Context(device=0, n_slots=48, n_coders=16, n_groups=6)
imgs = [pkg.syn1(H, W, 1 + k) for k in range(N)]
t0 = time.perf_counter()
pairs = ctx.encode_batch_indexed(imgs, R)
encode_s = time.perf_counter() - t0
assert all(ix is not None for _, ix in pairs)
split = {}


def leg_a():
    return [ctx.decode_indexed(s, ix) for s, ix in pairs]


def leg_a_thr():
    out, lock, todo = [None] * N, threading.Lock(), list(range(N))

    def work():
        while True:
            with lock:
                if not todo:
                    return
                k = todo.pop()
            out[k] = ctx.decode_indexed(*pairs[k])
    threads = [threading.Thread(target=work) for _ in range(min(16, N))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return out


def leg_b():
    return ctx.decode_batch_indexed(pairs)


def leg_rows_a():
    return [ctx.decode_rows(s, ix, *ROWS) for s, ix in pairs]


def leg_rows_b():
    return ctx.decode_batch_indexed(pairs, [ROWS] * N)


legs = {"a": leg_a, "a_thr": leg_a_thr, "b": leg_b}
row_legs = {"rows_a": leg_rows_a, "rows_b": leg_rows_b} if args.setting != "large" else {}


def run(name):
    fn = legs.get(name) or row_legs[name]
    t0 = time.perf_counter()
    res = fn()
    wall = time.perf_counter() - t0
    want = imgs if name in legs else [i[ROWS[0]:ROWS[1]] for i in imgs]
    assert len(res) == N and all(r is not None and (r == w).all() for r, w in zip(res, want)), name      # every plane against its input
    rec = {"leg": name, "wall_s": round(wall, 4)}
    if name in ("b", "rows_b"):
        rec["split_ms"] = {k: round(v, 2) for k, v in ctx.indexed_decode_split().items()}
    print(json.dumps(rec), flush=True)
    return rec


names = list(legs) + list(row_legs)
warm = [run(name) for name in names]
runs = [run(name) for _ in range(args.repeat) for name in names]
ctx.close()
summary = summarise(runs, list(legs), N * H * W)
summary.update(summarise(runs, list(row_legs), N * (ROWS[1] - ROWS[0]) * W))
doc = {"what": "indexed streams read back: decode_indexed per image in turn (a), one thread per image, 16 at a time (a_thr), one decode_batch_indexed "
               "call (b); streams and indexes from encode_batch_indexed on SYN-1 frames, seeds 1..N; same box, same process, context of 6 groups x 8 slots "
               "and 16 coder threads; one warm-up per leg, then the runs alternating; every plane compared with its input",
       "frames": N, "h": H, "w": W, "every_rows": R, "segments": N * ((H - 1) // R + 1), "stream_bytes": sum(len(s) for s, _ in pairs),
       "index_bytes": sum(len(ix) for _, ix in pairs), "encode_batch_indexed_s": round(encode_s, 3), "lib": os.environ.get("NBLIC_AMD_LIB", "in-tree"),
       "warm_up": warm, "runs": runs, "summary": summary, "b_against_a_thr": verdict(summary, "a_thr", "b")}
if row_legs:
    doc["rows"] = list(ROWS)
    doc["rows_b_against_rows_a"] = verdict(summary, "rows_a", "rows_b")
print(json.dumps({k: v for k, v in doc.items() if k.endswith("_a") or k.endswith("_thr")}), flush=True)
merge(args.setting, doc)
