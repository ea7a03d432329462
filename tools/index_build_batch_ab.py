"""Same-box A/B of three ways to index a batch of streams, in one process on one GPU:

  a        Context.build_index for each stream in turn;
  a_thr    16 threads, one build_index call each at a time: the most a caller could overlap before;
  b        one Context.build_index_batch call (planes wanted).

Streams come from Context.encode_modes on SYN-1 frames, seeds 1..N.  One warm-up per leg, then --repeat runs per leg,
alternating; wall time per run; every index of every run is compared with the first run's (leg a's warm-up), and every
plane of leg b with its input where the mode is lossless.  A leg whose warm-up takes more than a minute is not run again:
that one run is its time (no spread).  Leg b also reports where the call spent its time (Context.index_build_split: host
checks, uploads, the decode-and-capture launches, the finish).  Two settings:

  full     192 frames of 512 x 512, -n0 -e1, at R = 32: one class of at most 256 jobs, the decoders' full image;
  lean     512 frames of 256 x 256 at R = 32, the modes -n0 -e1, -n2 -e1, -n0 -e2, -n0 -e1, -n2 -e1, -n3 -e3 in turn: the
           -e1 class has 342 jobs, more than 256, and so takes the decoders' lean image; -e2 and -e3 have 85 each.

Each setting is one process; run each under its own time limit and chain them, so that a fault ends the sequence:

    timeout -k 10 600 python tools/index_build_batch_ab.py --setting full --out profiles/r15_index_build_batch_ab.json && \\
    timeout -k 10 600 python tools/index_build_batch_ab.py --setting lean --out profiles/r15_index_build_batch_ab.json

A setting's result is merged into --out under its name.  --bench NAME=FILE ... merges the JSON lines of bench.py runs
(one file per library) into the same document and exits.
"""
import argparse, importlib, json, os, statistics, sys, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--setting", choices=("full", "lean", "quick"), default="full")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--frames", type=int, default=0, help="override the setting's number of frames")
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


if args.bench is not None:
    lines = {}
    for item in args.bench:
        name, _, path = item.partition("=")
        with open(path) as f:
            lines[name] = [json.loads(l) for l in f if l.strip().startswith("{")]
    merge("bench", lines)
    sys.exit(0)

pkg = importlib.import_module("nblic-image-compression_amd")
E1 = [(0, 1)]
MIXED = [(0, 1), (2, 1), (0, 2), (0, 1), (2, 1), (3, 3)]
N, H, W, R, MODES = {"full": (192, 512, 512, 32, E1), "lean": (512, 256, 256, 32, MIXED), "quick": (12, 96, 128, 8, MIXED)}[args.setting]
N = args.frames or N
ctx = pkg.Context(device=0, n_slots=48, n_coders=16, n_groups=6)
imgs = [pkg.syn1(H, W, 1 + k) for k in range(N)]
modes = [MODES[k % len(MODES)] for k in range(N)]
t0 = time.perf_counter()
streams, _ = ctx.encode_modes(imgs, [m[0] for m in modes], [m[1] for m in modes], want_recon=False)
encode_s = time.perf_counter() - t0
e1_jobs = sum(1 for m in modes if m[1] == 1)
first = {}


def leg_a():
    return [ctx.build_index(s, R) for s in streams], None


def leg_a_thr():
    out, lock, todo = [None] * N, threading.Lock(), list(range(N))

    def work():
        while True:
            with lock:
                if not todo:
                    return
                k = todo.pop()
            out[k] = ctx.build_index(streams[k], R)
    threads = [threading.Thread(target=work) for _ in range(min(16, N))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return out, None


def leg_b():
    return ctx.build_index_batch(streams, R, planes=True)


legs = {"a": leg_a, "a_thr": leg_a_thr, "b": leg_b}


def run(name):
    t0 = time.perf_counter()
    indexes, planes = legs[name]()
    wall = time.perf_counter() - t0
    if "indexes" not in first:
        first["indexes"] = indexes
    assert len(indexes) == N and all(ix is not None and ix == f for ix, f in zip(indexes, first["indexes"])), name    # every index against the first run's
    if planes is not None:
        assert all(p is not None and (m[0] != 0 or (p == i).all()) for p, i, m in zip(planes, imgs, modes)), name   # lossless: the plane is the input
    rec = {"leg": name, "wall_s": round(wall, 4)}
    if name == "b":
        rec["split_ms"] = {k: round(v, 2) for k, v in ctx.index_build_split().items()}
    print(json.dumps(rec), flush=True)
    return rec


warm = [run(name) for name in legs]
once = [r["leg"] for r in warm if r["wall_s"] > 60.0]                   # a minute and more: the warm-up is the leg's one timed run
runs = [run(name) for _ in range(args.repeat) for name in legs if name not in once]
ctx.close()
summary = {}
for name in legs:
    t = [r["wall_s"] for r in (warm if name in once else runs) if r["leg"] == name]
    summary[name] = {"runs_s": t, "median_s": round(statistics.median(t), 4), "min_s": min(t), "max_s": max(t), "spread_s": round(max(t) - min(t), 4),
                     "median_mpixel_per_s": round(N * H * W / statistics.median(t) / 1e6, 1)}
splits = [r["split_ms"] for r in (warm if "b" in once else runs) if r["leg"] == "b"]
summary["b"]["split_ms_median"] = {k: round(statistics.median(s[k] for s in splits), 2) for k in splits[0]}
gain = summary["a_thr"]["median_s"] - summary["b"]["median_s"]
spread = max(summary["a_thr"]["spread_s"], summary["b"]["spread_s"])
doc = {"what": "streams indexed: build_index per stream in turn (a), 16 threads of build_index (a_thr), one build_index_batch call with planes (b); "
               "streams from encode_modes on SYN-1 frames, seeds 1..N; same box, same process, context of 6 groups x 8 slots and 16 coder threads; one "
               "warm-up per leg, then the runs alternating (a leg whose warm-up exceeds a minute: that one run); every index compared with the first "
               "run's, every lossless plane of b with its input",
       "frames": N, "h": H, "w": W, "every_rows": R, "modes_in_turn": [list(m) for m in MODES], "entries": N * ((H - 1) // R),
       "e1_class_jobs": e1_jobs, "e1_class_takes_the_lean_image": bool(pkg.serial_plan(True, 1, e1_jobs, W) & 2),
       "stream_bytes": sum(len(s) for s in streams), "index_bytes": sum(len(ix) for ix in first["indexes"]), "encode_modes_s": round(encode_s, 3),
       "lib": os.environ.get("NBLIC_AMD_LIB", "in-tree"), "timed_once": once, "warm_up": warm, "runs": runs, "summary": summary,
       "b_against_a_thr": {"ratio_of_medians": round(summary["a_thr"]["median_s"] / summary["b"]["median_s"], 2), "gain_s": round(gain, 4),
                           "larger_spread_s": spread, "gain_exceeds_three_spreads": bool(gain > 3 * spread)}}
print(json.dumps({"summary": summary, "b_against_a_thr": doc["b_against_a_thr"]}), flush=True)
merge(args.setting, doc)
