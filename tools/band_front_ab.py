"""Same-box A/B of the band encoder's two fronts (Context.stream(..., front="serial" | "staged")) on lossless -e1: per shape
one warm-up encode per front, then --repeat encodes per front, alternating, in one process.  Per run: wall time of the
whole encode, model_kernel_ms (the serial model kernel / the launches that replace it), bands, and the stream's SHA-256,
which must be the serial front's and -- for a shape the golden manifest knows -- the golden hash.  The index of every run
must be the first run's.  Writes one JSON document.

    python tools/band_front_ab.py --out profiles/r09_band_front_ab.json
"""
import argparse, hashlib, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--band-rows", type=int, default=64)
ap.add_argument("--index-every", type=int, default=64)
ap.add_argument("--quick", action="store_true", help="small images (a check of the tool, not a measurement)")
args = ap.parse_args()
pkg = importlib.import_module("nblic-image-compression_amd")
ctx = pkg.Context(device=0, n_slots=2, n_coders=2)
shapes = [(4096, 4096), (1024, 16384)]
if args.quick:
    shapes = [(512, 512), (128, 1024)]
with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
    golden = json.load(f)["large"]


def encode(img, front):
    t0 = time.perf_counter()
    enc = ctx.stream(img, 0, 1, band_rows=args.band_rows, index_every=args.index_every, front=front)
    try:
        done, s = enc.run()
        assert done
        wall = time.perf_counter() - t0
        prog, ix = enc.progress(), enc.index()
    finally:
        enc.close()
    assert prog["sha256"] == hashlib.sha256(s).hexdigest()
    return {"front": front, "wall_s": round(wall, 4), "model_kernel_ms": round(prog["model_kernel_ms"], 3), "sha256": prog["sha256"],
            "stream_bytes": len(s), "index_sha256": hashlib.sha256(ix).hexdigest(), "index_bytes": len(ix)}


def band_count(h):
    """Bands the encoder cuts h rows into: band_rows at a time, and never across an entry row of the index."""
    n = i = 0
    while i < h:
        rows = min(args.band_rows, h - i)
        if args.index_every > 0:
            rows = min(rows, args.index_every - i % args.index_every)
        i, n = i + rows, n + 1
    return n


doc = {"what": "band encoder, -n0 -e1, SYN-1: serial front (one-wave model kernel) against the staged front (key-partitioned kernels) "
               "on the same image, same box, same process; per shape one warm-up encode per front, then the runs alternating",
       "band_rows": args.band_rows, "index_every": args.index_every, "lib": os.environ.get("NBLIC_AMD_LIB", "in-tree"), "cases": []}
for h, w in shapes:
    img = pkg.syn1(h, w, 1)
    bands = band_count(h)
    before = ctx.serial_launches()
    warm = {front: encode(img, front) for front in ("serial", "staged")}
    assert ctx.serial_launches() - before == bands                 # the serial encode's bands; the staged one launched no model kernel
    runs = [encode(img, front) for _ in range(args.repeat) for front in ("serial", "staged")]
    ref = warm["serial"]
    for r in [warm["staged"]] + runs:
        assert (r["sha256"], r["index_sha256"]) == (ref["sha256"], ref["index_sha256"]), r
    g = golden.get(f"syn1s1_{h}x{w}_n0_e1")
    assert g or (h, w) != (4096, 4096), "the golden manifest has no 4096x4096 -n0 -e1 entry"
    if g:
        assert (ref["stream_bytes"], ref["sha256"]) == (g["len"], g["sha256"])
    best = {front: min((r for r in runs if r["front"] == front), key=lambda r: r["wall_s"]) for front in ("serial", "staged")}
    case = {"h": h, "w": w, "near": 0, "effort": 1, "bands": bands, "stream_bytes": ref["stream_bytes"], "sha256": ref["sha256"],
            "golden_sha256": bool(g), "index_bytes": ref["index_bytes"], "warm_up": [warm["serial"], warm["staged"]], "runs": runs,
            "best": {front: {"wall_s": b["wall_s"], "model_kernel_ms": b["model_kernel_ms"],
                             "mpixel_per_s": round(h * w / b["wall_s"] / 1e6, 1)} for front, b in best.items()},
            "wall_speedup": round(best["serial"]["wall_s"] / best["staged"]["wall_s"], 2),
            "model_stage_speedup": round(best["serial"]["model_kernel_ms"] / best["staged"]["model_kernel_ms"], 1)}
    print(json.dumps({k: v for k, v in case.items() if k not in ("runs", "warm_up")}), flush=True)
    doc["cases"].append(case)
ctx.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
