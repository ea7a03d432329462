"""Same-box A/B of the two ways to get a batch of effort-0 (QNBLIC) streams WITH their seek indexes, in one process on one GPU:

  plain      Context.qencode_batch alone: no index (what the index costs is read against it);
  two_call   Context.qencode_batch, then Context.build_index_batch on its streams: one serial decode of every stream;
  one_call   one Context.qencode_batch_indexed call.

One warm-up per leg, then --repeat runs per leg, alternating; wall time per run.  Every stream and every index of one
repetition is compared byte for byte between two_call and one_call, and every stream with plain's.  one_call also reports
where its group steps spent their time (Context.indexed_batch_split).  Two settings, each one process; run each under its own
time limit and chain them, so that a fault ends the sequence:

    timeout -k 10 900 python tools/qindexed_batch_ab.py --setting large --out profiles/r20_qindexed_batch_ab.json && \\
    timeout -k 10 600 python tools/qindexed_batch_ab.py --setting small --out profiles/r20_qindexed_batch_ab.json

  large    48 SYN-1 frames of 4096 x 4096 at R = 64 (seeds 1 .. 8 in turn);
  small    192 SYN-1 frames of 512 x 512 at R = 32.

A setting's result is merged into --out under its name.
"""
import argparse, importlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--setting", choices=("large", "small", "quick"), default="large")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--frames", type=int, default=0, help="override the setting's number of frames")
args = ap.parse_args()
pkg = importlib.import_module("nblic-image-compression_amd")
N, H, W, R = {"large": (48, 4096, 4096, 64), "small": (192, 512, 512, 32), "quick": (12, 96, 128, 16)}[args.setting]
N = args.frames or N
ctx = pkg.Context(device=0, n_slots=48, n_coders=16, n_groups=6)           # 6 groups x 8 slots
seeds = [pkg.syn1(H, W, s) for s in range(1, 9)]
imgs = [seeds[k % 8] for k in range(N)]


def leg_plain():
    return [(s, None) for s in ctx.qencode_batch(imgs)]


def leg_two_call():
    streams = ctx.qencode_batch(imgs)
    return list(zip(streams, ctx.build_index_batch(streams, R)))


def leg_one_call():
    return ctx.qencode_batch_indexed(imgs, R)


legs = {"plain": leg_plain, "two_call": leg_two_call, "one_call": leg_one_call}
compared = 0


def run(name, keep):
    global compared
    t0 = time.perf_counter()
    res = legs[name]()
    wall = time.perf_counter() - t0
    assert len(res) == N and all(s is not None for s, _ in res)
    if name != "plain":
        assert all(ix is not None for _, ix in res), name
    if "two_call" in keep and name == "one_call":                         # this repetition's two routes, byte for byte
        assert res == keep["two_call"], "the two routes differ"
        compared += 1
    if "plain" in keep and name != "plain":
        assert [s for s, _ in res] == [s for s, _ in keep["plain"]], name
    keep[name] = res
    rec = {"leg": name, "wall_s": round(wall, 4), "mpixel_per_s": round(N * H * W / wall / 1e6, 1)}
    if name == "one_call":
        rec["split"] = {k: round(v, 2) if isinstance(v, float) else v for k, v in ctx.indexed_batch_split().items()}
    print(json.dumps(rec), flush=True)
    return rec


keep = {}
warm = [run(name, keep) for name in legs]
stream_bytes = sum(len(s) for s, _ in keep["one_call"])
index_bytes = sum(len(ix) for _, ix in keep["one_call"])
runs = []
for _ in range(args.repeat):
    keep = {}
    runs += [run(name, keep) for name in legs]
ctx.close()
summary = {}
for name in legs:
    t = [r["wall_s"] for r in runs if r["leg"] == name]
    summary[name] = {"runs_s": t, "median_s": round(statistics.median(t), 4), "min_s": min(t), "max_s": max(t), "spread_s": round(max(t) - min(t), 4),
                     "median_mpixel_per_s": round(N * H * W / statistics.median(t) / 1e6, 1)}
gain = summary["two_call"]["median_s"] - summary["one_call"]["median_s"]
doc = {"what": "effort-0 (QNBLIC) streams with their seek indexes, SYN-1 seeds 1 .. 8 in turn: qencode_batch alone (plain), qencode_batch then "
               "build_index_batch (two_call), one qencode_batch_indexed call (one_call); same box, same process, context of 6 groups x 8 slots and "
               "16 coder threads; one warm-up per leg, then the runs alternating; every stream and index of a repetition compared between the routes",
       "frames": N, "h": H, "w": W, "every_rows": R, "stream_bytes": stream_bytes, "index_bytes": index_bytes, "repetitions_compared": compared,
       "lib": os.environ.get("NBLIC_AMD_LIB", "in-tree"), "warm_up": warm, "runs": runs, "summary": summary,
       "one_call_over_two_call": {"ratio_of_medians": round(summary["two_call"]["median_s"] / summary["one_call"]["median_s"], 2), "gain_s": round(gain, 4),
                                  "spread_of_two_call_s": summary["two_call"]["spread_s"], "gain_exceeds_spread": gain > summary["two_call"]["spread_s"]},
       "price_of_the_index": {"one_call_over_plain": round(summary["one_call"]["median_s"] / summary["plain"]["median_s"], 2)}}
print(json.dumps(doc["one_call_over_two_call"]), flush=True)
if args.out:
    full = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            full = json.load(f)
    full[args.setting] = doc
    with open(args.out, "w") as f:
        json.dump(full, f, indent=1)
        f.write("\n")
