"""Same-box A/B of three ways to get a batch of lossless -e1 streams WITH their seek indexes, in one process on one GPU:

  a        one band encoder after another (Context.stream(front="staged", index_every=R)), one image per object;
  a_six    the same, six objects at a time on six threads (a context of six groups: the most a caller can overlap);
  b        one Context.encode_batch_indexed call.

One warm-up per leg, then --repeat runs per leg, alternating; wall time per run.  Every stream of every run is held to the
golden hash of the frame (tests/golden/manifest.json) and every index to the first run's.  Leg b also reports where its
group steps spent their time (Context.indexed_batch_split).  Writes one JSON document.

    python tools/indexed_batch_ab.py --out profiles/r11_indexed_batch_ab.json
"""
import argparse, hashlib, importlib, json, os, statistics, sys, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--every-rows", type=int, default=64)
ap.add_argument("--quick", action="store_true", help="small frames (a check of the tool, not a measurement)")
args = ap.parse_args()
pkg = importlib.import_module("nblic-image-compression_amd")
H, W = (512, 512) if args.quick else (4096, 4096)
R, N = args.every_rows, args.frames
ctx = pkg.Context(device=0, n_slots=48, n_coders=16, n_groups=6)           # 6 groups x 8 slots
img = pkg.syn1(H, W, 1)
with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
    golden = json.load(f)["large"].get(f"syn1s1_{H}x{W}_n0_e1")
assert golden or args.quick, "the golden manifest has no entry for this frame"
sha = lambda b: hashlib.sha256(b).hexdigest()


def one_stream(_=None):
    enc = ctx.stream(img, 0, 1, index_every=R, front="staged")
    try:
        done, s = enc.run()
        assert done
        return sha(s), len(s), sha(enc.index())
    finally:
        enc.close()


def leg_a():
    return [one_stream() for _ in range(N)]


def leg_a_six():
    out, lock, todo = [], threading.Lock(), list(range(N))

    def work():
        while True:
            with lock:
                if not todo:
                    return
                todo.pop()
            r = one_stream()
            with lock:
                out.append(r)
    threads = [threading.Thread(target=work) for _ in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return out


def leg_b():
    got = ctx.encode_batch_indexed([img] * N, R)
    return [(sha(s), len(s), sha(ix)) for s, ix in got]


legs = {"a": leg_a, "a_six": leg_a_six, "b": leg_b}
first = None


def run(name):
    global first
    t0 = time.perf_counter()
    res = legs[name]()
    wall = time.perf_counter() - t0
    assert len(res) == N
    first = first or res[0]
    for r in res:
        assert r == first, (name, r, first)                               # same stream, same index, every frame of every run
        assert not golden or (r[1], r[0]) == (golden["len"], golden["sha256"]), (name, r)
    rec = {"leg": name, "wall_s": round(wall, 4), "mpixel_per_s": round(N * H * W / wall / 1e6, 1)}
    if name == "b":
        rec["split"] = {k: round(v, 2) if isinstance(v, float) else v for k, v in ctx.indexed_batch_split().items()}
    print(json.dumps(rec), flush=True)
    return rec


warm = [run(name) for name in legs]
runs = [run(name) for _ in range(args.repeat) for name in legs]
ctx.close()
summary = {}
for name in legs:
    t = [r["wall_s"] for r in runs if r["leg"] == name]
    summary[name] = {"runs_s": t, "median_s": round(statistics.median(t), 4), "min_s": min(t), "max_s": max(t), "spread_s": round(max(t) - min(t), 4),
                     "median_mpixel_per_s": round(N * H * W / statistics.median(t) / 1e6, 1)}
best_old = min(("a", "a_six"), key=lambda n: summary[n]["median_s"])
doc = {"what": "lossless -e1 streams with their seek indexes, SYN-1 seed 1: band encoders one after another (a), six at a time (a_six), "
               "one indexed batch call (b); same box, same process, context of 6 groups x 8 slots and 16 coder threads; one warm-up per leg, "
               "then the runs alternating; every stream held to the golden hash, every index to the first run's",
       "frames": N, "h": H, "w": W, "every_rows": R, "golden_sha256": bool(golden), "stream_sha256": first[0], "stream_bytes": first[1],
       "index_sha256": first[2], "lib": os.environ.get("NBLIC_AMD_LIB", "in-tree"), "warm_up": warm, "runs": runs, "summary": summary,
       "b_over_best_old": {"against": best_old, "ratio_of_medians": round(summary[best_old]["median_s"] / summary["b"]["median_s"], 2),
                           "gain_s": round(summary[best_old]["median_s"] - summary["b"]["median_s"], 4), "spread_of_that_leg_s": summary[best_old]["spread_s"]}}
print(json.dumps(doc["b_over_best_old"]), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
