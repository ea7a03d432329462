"""Same-box A/B of the encoders' device inputs, -n0 -e1, on one GPU.

Leg 1, no regression on the old path: N contiguous uint8 frames on the device go through
  parent_ptrs   Context.encode_ptrs(on_device=True) on ANOTHER build of the library (--parent-lib, through NBLIC_AMD_LIB),
  tree_ptrs     the same call on this tree,
  tree_in_place Context.encode_src_ptrs on this tree: the _from call, every source used where it lies.
Leg 2, what collecting costs: the same frames arrive as a 1-column crop of a pitched surface, as float16 channels-last with
scale = 255, and as interleaved RGB (three sources a frame); each goes through the _from call (crop_from, f16_from, rgb_from)
and through the torch expression of the same conversion into contiguous planes followed by encode_ptrs (crop_torch,
f16_torch, rgb_torch).  The _from legs record Context.collect_stats and the k_collect time (Context.collect_ms, HIP events
around the launches, enable_timing on) of one EXTRA, untimed run.

Without --leg the tool is the driver: it starts no GPU work itself and runs every (leg, repetition) as a child process with
a time limit of its own -- a library is chosen when the package is imported, so the two builds cannot share a process --
alternating the legs, --repeat times; a child makes its inputs and a fresh context, runs one warm-up and one timed run, and
prints one JSON line.  A child that fails ends the driver.  Medians of the repetitions, min-to-max spreads next to every
figure, every leg's lengths and stream hash compared with its counterpart's.  Two settings:

  large    48 frames of 4096 x 4096 (SYN-1, seeds 1 .. 4 repeated);
  small    192 frames of 512 x 512.

    timeout -k 10 1100 python tools/encode_from_device_ab.py --setting large --parent-lib PARENT/libnblic_amd.so --out profiles/r23_encode_from_device_ab.json && \\
    timeout -k 10 700 python tools/encode_from_device_ab.py --setting small --parent-lib PARENT/libnblic_amd.so --out profiles/r23_encode_from_device_ab.json

A setting's result is merged into --out under its name.
"""
import argparse, hashlib, importlib, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--setting", choices=("large", "small", "quick"), default="large")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--parent-lib", default="")
ap.add_argument("--leg", default="")
ap.add_argument("--child-timeout", type=int, default=240)
args = ap.parse_args()

N, S = {"large": (48, 4096), "small": (192, 512), "quick": (6, 256)}[args.setting]
assert N % 3 == 0
OLD = ("parent_ptrs", "tree_ptrs", "tree_in_place")
COST = ("crop_torch", "crop_from", "f16_torch", "f16_from", "rgb_torch", "rgb_from")


def child(leg):
    import numpy as np
    import torch
    torch.cuda.init()                                   # (torch first: the library binds to the HIP runtime that is already loaded)
    pkg = importlib.import_module("nblic-image-compression_amd")
    base = [pkg.syn1(S, S, 1 + k) for k in range(min(N, 4))]
    frames = [base[k % len(base)] for k in range(N)]
    kind = leg.split("_")[0]
    shapes = [(S, S)] * N
    # the producer's tensors, made outside the timed region
    if kind == "crop":
        held = [torch.from_numpy(np.concatenate([np.zeros((S, 1), np.uint8), f], 1)).cuda() for f in frames]
        views, scale = [t[:, 1:] for t in held], 1.0
        planes_of = lambda: [v.contiguous() for v in views]
    elif kind == "f16":
        held = [torch.from_numpy(np.stack(frames[3 * n:3 * n + 3])[None]).cuda().to(torch.float16).div_(255).contiguous(memory_format=torch.channels_last)
                for n in range(N // 3)]                     # [1, 3, H, W] each, channels last
        views, scale = [t[0][c] for t in held for c in range(3)], 255.0
        planes_of = lambda: [(v.float() * 255.0).round_().clamp_(0, 255).to(torch.uint8).contiguous() for v in views]
    elif kind == "rgb":
        held = [torch.from_numpy(np.stack(frames[3 * n:3 * n + 3], -1)).cuda() for n in range(N // 3)]
        views, scale = [t[:, :, c] for t in held for c in range(3)], 1.0
        planes_of = lambda: [p for t in held for p in t.permute(2, 0, 1).contiguous()]
    else:
        held = [torch.from_numpy(f).cuda() for f in frames]
        views, scale = held, 1.0
        planes_of = lambda: held
    if kind == "f16":                                   # (k / 255 in float16, times 255, rounds back to k: the same planes as every other leg)
        assert all(v.stride()[1] == 3 for v in views)
    torch.cuda.synchronize()
    outs = [np.empty(pkg.out_capacity(S, S), np.uint8) for _ in range(N)]
    for o in outs:
        o[::4096] = 0                                   # touched once: no leg pays for the first fault of a page
    from_call = leg.endswith("_from") or leg == "tree_in_place"
    if from_call:
        srcs, fmt = pkg._srcs_of(views, None, None)

    def once(ctx):
        if from_call:
            return ctx.encode_src_ptrs(srcs, fmt, scale, 0.0, outs)
        planes = planes_of()
        torch.cuda.synchronize()
        return ctx.encode_ptrs([p.data_ptr() for p in planes], shapes, True, outs)

    ctx = pkg.Context(device=0, n_slots=48, n_coders=16, n_groups=6)
    rec = {"leg": leg, "lib": "--parent-lib" if os.environ.get("NBLIC_AMD_LIB") else "in-tree"}
    try:
        once(ctx)                                       # warm-up
        s0 = ctx.collect_stats() if from_call else None
        t0 = time.perf_counter()
        got, lens = once(ctx)
        rec["wall_s"] = round(time.perf_counter() - t0, 4)
        if from_call:
            rec["collect_stats"] = [b - a for a, b in zip(s0, ctx.collect_stats())]
            ctx.enable_timing(True)                     # one extra run, not timed by the clock: the k_collect launches between events
            once(ctx)
            ms, timed = ctx.collect_ms()
            rec["k_collect_ms"], rec["k_collect_launches_timed"] = round(ms, 3), timed
            stages = list(ctx.stage_times().items())     # in launch order: the front half ends where the host sizes the back half
            gap = [k for k, _ in stages].index("host_gap")
            rec["front_half_ms_of_that_run"] = round(sum(v for _, v in stages[:gap]), 2)
    finally:
        ctx.close()
    h = hashlib.sha256()
    for o, n in zip(got, lens):
        h.update(o[:int(n)].tobytes())
    rec["stream_bytes"], rec["streams_sha256"] = int(lens.sum()), h.hexdigest()
    rec["mpixel_per_s"] = round(N * S * S / rec["wall_s"] / 1e6, 1)
    print("RESULT " + json.dumps(rec), flush=True)


def run_child(leg):
    env = dict(os.environ)
    env.pop("NBLIC_AMD_LIB", None)
    if leg == "parent_ptrs":
        env["NBLIC_AMD_LIB"] = os.path.abspath(args.parent_lib)
    cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--setting", args.setting, "--leg", leg]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:                   # a fault, a time limit, a failed check: nothing more is started
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"leg {leg} ended with status {r.returncode}: the A/B stops here")
    rec = json.loads(line[0][len("RESULT "):])
    print(json.dumps(rec), flush=True)
    return rec


def summarise(runs, legs):
    out = {}
    for name in legs:
        mine = [r for r in runs if r["leg"] == name]
        t = [r["wall_s"] for r in mine]
        out[name] = {"runs_s": t, "median_s": round(statistics.median(t), 4), "min_s": min(t), "max_s": max(t), "spread_s": round(max(t) - min(t), 4),
                     "mpixel_per_s_of_median": round(N * S * S / statistics.median(t) / 1e6, 1)}
        if "k_collect_ms" in mine[0]:
            out[name]["collect_stats"] = mine[0]["collect_stats"]
            out[name]["k_collect_ms_median"] = round(statistics.median(r["k_collect_ms"] for r in mine), 3)
            out[name]["k_collect_launches_timed"] = mine[0]["k_collect_launches_timed"]
            out[name]["front_half_ms_median"] = round(statistics.median(r["front_half_ms_of_that_run"] for r in mine), 2)
    return out


if args.leg:
    child(args.leg)
    sys.exit(0)

legs = (OLD if args.parent_lib else OLD[1:]) + COST
runs = [run_child(leg) for _ in range(args.repeat) for leg in legs]
assert len({(r["stream_bytes"], r["streams_sha256"]) for r in runs}) == 1, "the legs' streams differ"
summary = summarise(runs, legs)
doc = {"what": "-n0 -e1 encode of N uint8 frames that lie on the device: encode_ptrs(on_device=True) on the parent commit's library (parent_ptrs) and on this "
               "tree (tree_ptrs), the _from call with every source in place (tree_in_place); and the frames as a 1-column crop of a pitched surface, as "
               "float16 channels-last (scale 255) and as interleaved RGB through the _from call (x_from) against the torch expression of the conversion "
               "followed by encode_ptrs (x_torch).  Same box; every (leg, repetition) a process of its own with a fresh context of 6 groups x 8 slots and "
               "16 coder threads, one warm-up and one timed run, the legs alternating; every leg's streams are the same bytes",
       "frames": N, "h": S, "w": S, "repeat": args.repeat, "runs": runs, "summary": summary}
if args.parent_lib:
    spread = summary["parent_ptrs"]["spread_s"]
    doc["leg_1"] = {"parent_spread_s": spread,
                    **{name: {"slower_than_parent_by_s": round(summary[name]["median_s"] - summary["parent_ptrs"]["median_s"], 4),
                              "within_parent_spread": bool(summary[name]["median_s"] - summary["parent_ptrs"]["median_s"] <= spread)} for name in OLD[1:]}}
doc["leg_2"] = {k: {"from_over_torch_ratio_of_medians": round(summary[k + "_torch"]["median_s"] / summary[k + "_from"]["median_s"], 3),
                    "gain_s": round(summary[k + "_torch"]["median_s"] - summary[k + "_from"]["median_s"], 4), "spread_of_torch_leg_s": summary[k + "_torch"]["spread_s"],
                    "k_collect_over_front_half": round(summary[k + "_from"]["k_collect_ms_median"] / max(summary[k + "_from"]["front_half_ms_median"], 1e-9), 4)}
                for k in ("crop", "f16", "rgb")}
print(json.dumps({k: doc[k] for k in doc if k.startswith("leg_")}), flush=True)
if args.out:
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.load(f)
    merged[args.setting] = doc
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")
