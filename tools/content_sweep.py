"""Throughput by CONTENT: what the staged -n0 -e1 / effort-0 pipeline makes of frames on which one table entry holds most
of the pixels (flat, saturated, document-like, dark), next to SYN-1 -- the one texture every other figure was taken on.

Legs (4096 x 4096 frames, integer generators, fixed seeds):
  syn1 const sat255 checker ramp half-flat document dark-noise    Context.encode_batch of FRAMES frames of the class
  mixed        groups of seven SYN-1 frames and one const frame (a group of eight shares every launch)
  q-const      Context.qencode_batch (effort 0) on const
  band-const   Context.encode_batch_indexed at R = 64 on const

One leg is one fresh process (--leg NAME): a warm-up call, REPEAT timed calls, then one call with every stage timed;
prints one JSON line: Mpx/s, stage_times per launch, long_chain_stats with the S3 hit rate, the streams' hashes, and a
1024 x 1024 sample of the class checked for equality against the compiled reference (oracle/_ref) where that exists.

Without --leg the tool is the driver: it starts no GPU work itself, runs every leg as a child with a time limit of its own,
LINES times, and -- with --parent-lib, another build of the library -- alternates each leg between this tree and that
build (NBLIC_AMD_LIB), so a build that takes seconds per flat frame cannot hold up the rest; that build runs
PARENT_FRAMES frames per call on every leg but syn1 and mixed.  Streams of the two builds must be the same bytes.  Writes one JSON document.

    python tools/content_sweep.py --parent-lib /path/to/libnblic_amd.so --out profiles/r16_content_sweep.json
"""
import argparse, hashlib, importlib, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = ["syn1", "const", "sat255", "checker", "ramp", "half-flat", "document", "dark-noise"]
LEGS = CLASSES + ["mixed", "q-const", "band-const"]

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=LEGS)
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--parent-frames", type=int, default=8, help="frames per call on --parent-lib, for every leg but syn1 and mixed")
ap.add_argument("--parent-repeat", type=int, default=1, help="timed calls per leg process on --parent-lib")
ap.add_argument("--earlier-lines", default="", help="a JSON document of an earlier run of other legs: its lines are summarised with this run's")
ap.add_argument("--repeat", type=int, default=3, help="timed calls per leg process")
ap.add_argument("--lines", type=int, default=3, help="processes per leg and build")
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--step-timeout", type=float, default=150.0, help="seconds one leg process may take")
ap.add_argument("--parent-lib", default="")
ap.add_argument("--legs", default=",".join(LEGS))
ap.add_argument("--out", default="")
args = ap.parse_args()


def frame(cls, h, w, seed):
    import numpy as np
    rng = np.random.default_rng(1000 + seed)
    if cls == "const":
        return np.full((h, w), 90 + seed % 64, np.uint8)
    if cls == "sat255":
        return np.full((h, w), 255, np.uint8)
    if cls == "checker":
        i, j = np.indices((h, w))
        return (((i >> 3) + (j >> 3) + seed) % 2 * 255).astype(np.uint8)
    if cls == "ramp":
        return np.broadcast_to(((np.arange(w) * 255) // max(w - 1, 1)).astype(np.uint8), (h, w)).copy()
    if cls == "half-flat":
        img = np.full((h, w), 60, np.uint8)
        img[h // 2:] = rng.integers(40, 90, (h - h // 2, w))
        return img
    if cls == "document":                                # white page, sparse dark strokes in text-like rows
        img = np.full((h, w), 250, np.uint8)
        for r in range(40, h - 40, 48):
            cols = rng.integers(0, w - 24, w // 40)
            for c in cols:
                img[r:r + int(rng.integers(8, 20)), c:c + int(rng.integers(2, 24))] = rng.integers(0, 60)
        return img
    if cls == "dark-noise":
        return rng.integers(0, 3, (h, w)).astype(np.uint8)
    raise ValueError(cls)


def run_leg():
    import numpy as np
    pkg = importlib.import_module("nblic-image-compression_amd")
    leg, S, N = args.leg, args.size, args.frames
    cls = {"mixed": "const", "q-const": "const", "band-const": "const"}.get(leg, leg)
    made = {}                                            # four distinct frames per class, handed over N times

    def one(c, seed):
        if (c, seed) not in made:
            made[(c, seed)] = pkg.syn1(S, S, 1 + seed) if c == "syn1" else frame(c, S, S, seed)
        return made[(c, seed)]
    if leg == "mixed":
        frames = [one("const", k % 4) if k % 8 == 7 else one("syn1", k % 4) for k in range(N)]
    else:
        frames = [one(cls, k % 4) for k in range(N)]
    ctx = pkg.Context(device=0, n_slots=min(48, max(8, N)), n_coders=16, n_groups=max(1, min(6, N // 8)))
    has_stats = hasattr(ctx.lib, "nblic_amd_long_chain_stats")
    call = {"q-const": ctx.qencode_batch, "band-const": lambda f: [s for s, _ in ctx.encode_batch_indexed(f, 64)]}.get(leg, ctx.encode_batch)
    sha = lambda b: hashlib.sha256(b).hexdigest()
    first = call(frames)                                 # warm-up; its streams are the ones every later call is held to
    if has_stats:
        ctx.long_chain_stats(reset=True)
    walls = []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        got = call(frames)
        walls.append(time.perf_counter() - t0)
        assert got == first
    rec = {"leg": leg, "lib": os.environ.get("NBLIC_AMD_LIB", "in-tree"), "frames": N, "size": S, "wall_s": [round(t, 4) for t in walls],
           "mpixel_per_s": round(N * S * S / statistics.median(walls) / 1e6, 1),
           "streams_sha256": sha(b"".join(first)), "bytes_per_frame": round(sum(map(len, first)) / N, 1)}
    if has_stats:
        st = ctx.long_chain_stats()
        st = {k: v // args.repeat for k, v in st.items()}            # per call
        tried = st["s3_accepted"] + st["s3_missed"]
        rec["long_chain_stats_per_call"] = st
        rec["s3_hit_rate"] = round(st["s3_accepted"] / tried, 4) if tried else None
    if leg not in ("q-const", "band-const"):             # one more call with an event around every launch
        ctx.enable_timing(1)
        call(frames)
        st, ln = ctx.stage_times(), max(1, ctx.last_launches())
        ctx.enable_timing(0)
        rec["stage_ms_per_launch"] = {k: round(v / ln, 3) for k, v in st.items() if v / ln >= 0.05}
        rec["stage_launches"] = ln
    # a sample of the class against the reference itself
    from oracle.oracle import Reference
    if Reference.available():
        ref = Reference()
        sample = np.ascontiguousarray((frames[7] if leg == "mixed" else frames[0])[:1024, :1024])
        if leg == "q-const":
            rec["sample_equals_reference"] = ctx.qencode_batch([sample])[0] == ref.qencode(sample)
        else:
            rec["sample_equals_reference"] = ctx.encode_batch([sample])[0] == ref.encode(sample, 0, 1)[0]
        assert rec["sample_equals_reference"]
    ctx.close()
    print(json.dumps(rec), flush=True)


def drive():
    legs = [l for l in args.legs.split(",") if l]
    builds = [("new", "")] + ([("parent", args.parent_lib)] if args.parent_lib else [])
    lines = []
    if args.earlier_lines:
        with open(args.earlier_lines) as f:
            lines = json.load(f)["lines"]
        legs = list(dict.fromkeys([r["leg"] for r in lines] + legs))
    todo = [l for l in args.legs.split(",") if l]
    for leg in todo:
        for _ in range(args.lines):
            for name, lib in builds:                     # alternating: new, parent, new, parent, ...
                n = args.parent_frames if name == "parent" and leg not in ("syn1", "mixed") else args.frames
                env = dict(os.environ)
                env.pop("NBLIC_AMD_LIB", None)
                if lib:
                    env["NBLIC_AMD_LIB"] = lib
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--frames", str(n), "--size", str(args.size),
                       "--repeat", str(args.parent_repeat if name == "parent" else args.repeat)]
                t0 = time.perf_counter()
                try:
                    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.step_timeout)
                    out = [l for l in p.stdout.splitlines() if l.startswith("{")]
                    rec = json.loads(out[-1]) if p.returncode == 0 and out else {"leg": leg, "failed": p.returncode, "stderr": p.stderr[-400:]}
                except subprocess.TimeoutExpired:
                    rec = {"leg": leg, "timed_out_after_s": args.step_timeout, "frames": n, "failed": -9}
                rec["build"] = name
                rec["process_s"] = round(time.perf_counter() - t0, 1)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                finish(lines, legs, builds, stopped="not finished")              # the document is current after every line
                if "failed" in rec and rec["failed"] < 0:            # a child died on a signal or ran into its limit: nothing more is started on this card
                    return finish(lines, legs, builds, stopped=f"{leg} ({name}) ended with {rec['failed']}")
    return finish(lines, legs, builds)


def finish(lines, legs, builds, stopped=None):
    summary = {}
    for leg in legs:
        row = {}
        for name, _ in builds:
            ok = [r for r in lines if r["leg"] == leg and r["build"] == name and "mpixel_per_s" in r]
            if not ok:
                row[name] = {"lines": 0, "not_finished": len([r for r in lines if r["leg"] == leg and r["build"] == name])}
                continue
            v = [r["mpixel_per_s"] for r in ok]
            row[name] = {"lines_mpixel_per_s": v, "median_mpixel_per_s": statistics.median(v), "min": min(v), "max": max(v), "frames": ok[0]["frames"],
                         "streams_sha256": ok[0]["streams_sha256"]}
            for k in ("long_chain_stats_per_call", "s3_hit_rate", "stage_ms_per_launch", "sample_equals_reference"):
                if k in ok[-1]:
                    row[name][k] = ok[-1][k]
        if "median_mpixel_per_s" in row.get("new", {}) and "median_mpixel_per_s" in row.get("parent", {}):
            n, p = row["new"], row["parent"]
            row["new_over_parent"] = round(n["median_mpixel_per_s"] / p["median_mpixel_per_s"], 2)
            row["gain_mpixel_per_s"] = round(n["median_mpixel_per_s"] - p["median_mpixel_per_s"], 1)
            row["parent_spread_mpixel_per_s"] = round(p["max"] - p["min"], 1)
            if n["frames"] == p["frames"]:
                row["same_streams"] = n["streams_sha256"] == p["streams_sha256"]        # the same bytes from both builds
        summary[leg] = row
    syn = summary.get("syn1", {}).get("new", {}).get("median_mpixel_per_s")
    if syn:
        for leg in legs:
            m = summary[leg].get("new", {}).get("median_mpixel_per_s")
            if m:
                summary[leg]["ratio_to_syn1"] = round(m / syn, 3)
    doc = {"what": "throughput by content class, 4096 x 4096 frames: Context.encode_batch per class, a mixed leg (seven SYN-1 frames and one const "
                   "frame per group of eight), qencode_batch and encode_batch_indexed (R = 64) on const; every leg a fresh process with one warm-up "
                   "call, the builds alternating line by line on one card, every process under a time limit of its own",
           "size": args.size, "frames": args.frames, "parent_frames": args.parent_frames, "repeat": args.repeat, "parent_repeat": args.parent_repeat, "lines_per_leg_and_build": args.lines,
           "parent_lib": bool(args.parent_lib), "stopped_early": stopped, "summary": summary, "lines": lines}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0 if stopped is None else 1


if __name__ == "__main__":
    if args.leg:
        run_leg()
    else:
        sys.exit(drive())
