"""Sizes of packed seek indexes, and a same-box A/B of decode_batch_indexed on them against the PARENT commit's library.

For each setting -- the image sets of profiles/r14_indexed_batch_decode_ab.json and profiles/r15_index_build_batch_ab.json:

  large    16 SYN-1 frames of 4096 x 4096, -n0 -e1, R = 64
  small    64 frames of 1024 x 1024, -n0 -e1, R = 32
  full     192 frames of 512 x 512, -n0 -e1, R = 32
  lean     512 frames of 256 x 256, -n0 -e1, -n2 -e1, -n0 -e2, -n0 -e1, -n2 -e1, -n3 -e3 in turn, R = 32

it records, per mode, the bytes of the streams, of their indexes and of the packed indexes, and times three legs of one
decode_batch_indexed call over the whole set:

  parent_unpacked   the parent's library (NBLIC_AMD_LIB=--parent-lib), unpacked indexes
  tree_unpacked     this tree's library, unpacked indexes
  tree_packed       this tree's library, packed indexes (checked packed on the host, expanded on the device)

A library is fixed when a process loads it, so every timed run is a fresh child process of this tool (one GPU process at a
time): parent, tree, parent, tree, ... --repeat times; a tree child times both of its legs, alternating, after one warm-up
of each.  Every child prints the SHA-256 of all planes it got, and all of them must agree.  A child that fails ends the run.

    timeout -k 10 1100 python tools/packed_index_ab.py --parent-lib ab/parent/libnblic_amd.so --out profiles/r17_packed_index.json
"""
import argparse, hashlib, importlib, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E1 = [(0, 1)]
MIXED = [(0, 1), (2, 1), (0, 2), (0, 1), (2, 1), (3, 3)]
SETTINGS = {"large": (16, 4096, 4096, 64, E1), "small": (64, 1024, 1024, 32, E1), "full": (192, 512, 512, 32, E1),
            "lean": (512, 256, 256, 32, MIXED), "quick": (12, 96, 128, 8, MIXED)}

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--parent-lib", default="")
ap.add_argument("--settings", nargs="*", default=["large", "small", "full", "lean"])
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--child", default="", help="internal: run one setting in this process and print one JSON line")
ap.add_argument("--child-timeout", type=int, default=240)
args = ap.parse_args()


def child(setting):
    pkg = importlib.import_module("nblic-image-compression_amd")
    n, h, w, r, modes_in_turn = SETTINGS[setting]
    tree = "NBLIC_AMD_LIB" not in os.environ
    ctx = pkg.Context(device=0, n_slots=48, n_coders=16, n_groups=6)
    imgs = [pkg.syn1(h, w, 1 + k) for k in range(n)]
    modes = [modes_in_turn[k % len(modes_in_turn)] for k in range(n)]
    if modes_in_turn == E1:
        pairs = ctx.encode_batch_indexed(imgs, r)
    else:
        streams, _ = ctx.encode_modes(imgs, [m[0] for m in modes], [m[1] for m in modes], want_recon=False)
        pairs = list(zip(streams, ctx.build_index_batch(streams, r)))
    assert all(ix is not None for _, ix in pairs)
    out = {"setting": setting, "lib": os.environ.get("NBLIC_AMD_LIB", "in-tree"), "runs": {}}
    legs = {"parent_unpacked": pairs} if not tree else {"tree_unpacked": pairs}
    if tree:
        t0 = time.perf_counter()
        packed = [(s, pkg.pack_index(ix)) for s, ix in pairs]
        out["pack_s"] = round(time.perf_counter() - t0, 3)
        assert all(pkg.unpack_index(p) == ix for (_, p), (_, ix) in zip(packed[:: max(1, n // 8)], pairs[:: max(1, n // 8)]))
        legs["tree_packed"] = packed
        sizes = {}
        for (s, ix), (_, p), m in zip(pairs, packed, modes):
            d = sizes.setdefault("-n%d -e%d" % m, {"frames": 0, "stream_bytes": 0, "index_bytes": 0, "packed_index_bytes": 0})
            d["frames"] += 1; d["stream_bytes"] += len(s); d["index_bytes"] += len(ix); d["packed_index_bytes"] += len(p)
        for d in sizes.values():
            d["packed_over_unpacked"] = round(d["packed_index_bytes"] / d["index_bytes"], 4)
            d["packed_over_stream"] = round(d["packed_index_bytes"] / d["stream_bytes"], 4)
        out["sizes"] = sizes

    def run(name):
        t0 = time.perf_counter()
        planes = ctx.decode_batch_indexed(legs[name])
        wall = time.perf_counter() - t0
        assert all(p is not None for p in planes), name
        sha = hashlib.sha256()
        for p in planes:
            sha.update(p.tobytes())
        return {"wall_s": round(wall, 4), "planes_sha256": sha.hexdigest(), "split_ms": {k: round(v, 2) for k, v in ctx.indexed_decode_split().items()}}

    out["warm_up"] = {name: run(name) for name in legs}
    for name in legs:
        out["runs"][name] = run(name)
    lossless = [k for k, m in enumerate(modes) if m[0] == 0]
    planes = ctx.decode_batch_indexed([legs[list(legs)[-1]][k] for k in lossless])
    assert all((p == imgs[k]).all() for p, k in zip(planes, lossless)), "a lossless plane differs from its input"
    ctx.close()
    print("CHILD " + json.dumps(out), flush=True)


if args.child:
    child(args.child)
    sys.exit(0)

doc = {}
if args.out and os.path.exists(args.out):
    with open(args.out) as f:
        doc = json.load(f)
for setting in args.settings:
    n, h, w, r, modes_in_turn = SETTINGS[setting]
    runs, shas, sizes, pack_s, children = {"parent_unpacked": [], "tree_unpacked": [], "tree_packed": []}, set(), None, None, []
    for rep in range(args.repeat):
        for lib in ("parent", "tree"):
            env = dict(os.environ)
            env.pop("NBLIC_AMD_LIB", None)
            if lib == "parent":
                env["NBLIC_AMD_LIB"] = os.path.abspath(args.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", setting], env=env, capture_output=True, text=True, timeout=args.child_timeout)
            line = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
                sys.exit("a child failed (%s, %s, exit %d): nothing more is started" % (setting, lib, p.returncode))
            c = json.loads(line[0][6:])
            children.append(c)
            for name, rec in c["runs"].items():
                runs[name].append(rec["wall_s"]); shas.add(rec["planes_sha256"])
            sizes, pack_s = c.get("sizes", sizes), c.get("pack_s", pack_s)
            print(setting, lib, {k: v["wall_s"] for k, v in c["runs"].items()}, flush=True)
    assert len(shas) == 1, "the legs did not decode the same planes"
    summary = {k: {"runs_s": t, "median_s": round(statistics.median(t), 4), "min_s": min(t), "max_s": max(t), "spread_s": round(max(t) - min(t), 4)} for k, t in runs.items()}
    spread = summary["parent_unpacked"]["spread_s"]
    verdicts = {}
    for name in ("tree_unpacked", "tree_packed"):
        slower = round(summary[name]["median_s"] - summary["parent_unpacked"]["median_s"], 4)
        verdicts[name] = {"slower_than_parent_by_s": slower, "parent_spread_s": spread, "within_parent_spread": bool(slower <= spread)}
    doc[setting] = {"what": "one decode_batch_indexed call over the set: the parent's library on unpacked indexes, this tree on unpacked, this tree on packed; a fresh "
                            "process per library, parent and tree alternating, one warm-up per leg in each process; all planes' SHA-256 equal across every run",
                    "frames": n, "h": h, "w": w, "every_rows": r, "modes_in_turn": [list(m) for m in modes_in_turn], "sizes_by_mode": sizes,
                    "pack_index_all_s": pack_s, "summary": summary, "against_parent": verdicts, "children": children}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps({"setting": setting, "sizes_by_mode": sizes, "summary": summary, "against_parent": verdicts}), flush=True)
