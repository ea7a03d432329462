"""A/B of the queue plan (csrc/queue_plan.h): python bench.py with the parent commit's library (through NBLIC_AMD_LIB) and
with this tree's, alternating in one call, three runs each, every run a process of its own under its own time limit.  One
leg per invocation, merged into --out under the leg's name:

    python tools/queue_plan_ab.py --leg line --parent-lib PARENT/libnblic_amd.so --out profiles/r29_queue_plan_ab.json
    python tools/queue_plan_ab.py --leg effort0 --bench-args "--effort 0 --steps 10 --warmup 3" ...
    python tools/queue_plan_ab.py --leg full_small --bench-args "--full --no-cpu-baseline --steps 3 --warmup 1 --h2d-steps 0" ...
    python tools/queue_plan_ab.py --leg line_q16 --queues 16 ...
    python tools/queue_plan_ab.py --leg line_switch --tree-only-switch ...     (this tree's library alone, NBLIC_AMD_QUEUE_PLAN=0 against unset)

Recorded per side: the line's value, and where the run printed them the single-frame milliseconds and the 8-frame rate;
median, min, max, spread.  `gain` holds the bar a default must clear: this tree's median above the parent's MAXIMUM, and
the difference of medians at least twice the parent's own min-to-max spread in this call.  --queues N sets
GPU_MAX_HW_QUEUES=N for the runs of this leg only (a setting of the process the library itself never touches).  Nothing
more is started on the GPU after a run that failed."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--leg", required=True)
ap.add_argument("--out", required=True)
ap.add_argument("--parent-lib", default="")
ap.add_argument("--bench-args", default="")
ap.add_argument("--queues", type=int, default=0)
ap.add_argument("--tree-only-switch", action="store_true", help="both sides run this tree's library: 'parent' with NBLIC_AMD_QUEUE_PLAN=0, 'tree' with it unset")
ap.add_argument("--plan-on", action="store_true", help="set NBLIC_AMD_QUEUE_PLAN=1 for the tree's runs (a tree whose default is off)")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--bench-limit", type=int, default=170, help="seconds one bench.py run may take")
args = ap.parse_args()
assert args.tree_only_switch or args.parent_lib, "--parent-lib is needed"

METRICS = ("value", "single_frame_ms", "batch8_Mpixel_per_s")


def find(d, key):
    if isinstance(d, dict):
        if key in d:
            return d[key]
        for v in d.values():
            r = find(v, key)
            if r is not None:
                return r
    return None


def stat(values):
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3),
            "spread": round(max(values) - min(values), 3), "runs": [round(v, 3) for v in values]}


runs = {"parent": [], "tree": []}
for k in range(args.runs):
    for side in ("parent", "tree"):
        env = dict(os.environ)
        for name in ("NBLIC_AMD_LIB", "NBLIC_AMD_QUEUE_PLAN"):
            env.pop(name, None)
        if args.queues:
            env["GPU_MAX_HW_QUEUES"] = str(args.queues)
        if side == "parent":
            if args.tree_only_switch:
                env["NBLIC_AMD_QUEUE_PLAN"] = "0"
            else:
                env["NBLIC_AMD_LIB"] = os.path.abspath(args.parent_lib)
        elif args.plan_on:
            env["NBLIC_AMD_QUEUE_PLAN"] = "1"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args.bench_args.split(), env=env, capture_output=True, text=True, timeout=args.bench_limit)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:])
            raise SystemExit(f"bench.py failed on the {side} side (rc {r.returncode})")
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        rec = {m: find(line, m) for m in METRICS}
        rec["bit_exact"] = line.get("bit_exact")
        rec["queue_plan_line"] = [l for l in r.stderr.splitlines() if "queue plan" in l][:1]
        runs[side].append(rec)
        print(side, k, rec, flush=True)

doc = {"what": "python bench.py " + args.bench_args + (f" with GPU_MAX_HW_QUEUES={args.queues}" if args.queues else "") + ": " +
               ("this tree's library with NBLIC_AMD_QUEUE_PLAN=0 ('parent') and unset ('tree')" if args.tree_only_switch else "the parent commit's library and this tree's") +
               f", alternating in one call, {args.runs} runs each", "runs": runs}
for m in METRICS:
    if all(r[m] is not None for side in runs.values() for r in side):
        doc[m] = {side: stat([float(r[m]) for r in runs[side]]) for side in runs}
p, t = doc["value"]["parent"], doc["value"]["tree"]
diff = round(t["median"] - p["median"], 3)
doc["gain"] = {"tree_median_minus_parent_median": diff, "percent": round(100.0 * diff / p["median"], 2), "parent_spread": p["spread"],
               "tree_median_above_parent_max": bool(t["median"] > p["max"]), "difference_at_least_twice_parent_spread": bool(diff >= 2.0 * p["spread"]),
               "difference_over_parent_spread": round(diff / p["spread"], 2) if p["spread"] > 0 else None,
               "within_parent_spread": bool(p["median"] - t["median"] <= p["spread"])}
doc["gain"]["counts_as_a_gain"] = doc["gain"]["tree_median_above_parent_max"] and doc["gain"]["difference_at_least_twice_parent_spread"]
checked = [r["bit_exact"] for side in runs.values() for r in side if r["bit_exact"] is not None]      # (a plain run checks nothing and prints null)
doc["all_bit_exact"] = all(v is True for v in checked) if checked else None

old = {}
if os.path.exists(args.out):
    with open(args.out) as f:
        old = json.load(f)
old[args.leg] = doc
with open(args.out, "w") as f:
    json.dump(old, f, indent=1)
    f.write("\n")
print(json.dumps({"leg": args.leg, "value": doc["value"], "gain": doc["gain"], "all_bit_exact": doc["all_bit_exact"]}))
