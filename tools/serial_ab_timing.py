"""-e2 / -e3 per-pixel times of ONE image (encode_modes / decode_batch of one image, host clock around the synchronous
call), repeated, for comparing two builds of the package: run it once per build, alternating, in one session.

    python tools/serial_ab_timing.py [--package-dir DIR] [--label NAME] [--size 512] [--repeats 5]

--package-dir: the directory that holds the `nblic-image-compression_amd` package to measure (a built checkout of
another commit); default: this tree.  Prints one JSON line.  profiles/r07_lsq_redo_counter_ab.json was made with it.
"""
import argparse, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--package-dir", default=ROOT)
ap.add_argument("--label", default="this tree")
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.abspath(args.package_dir))
import numpy as np
pkg = importlib.import_module("nblic-image-compression_amd")
assert os.path.dirname(os.path.dirname(os.path.abspath(pkg.__file__))) == os.path.abspath(args.package_dir), pkg.__file__
from oracle.oracle import syn1
H = W = args.size
ctx = pkg.Context(device=0, n_slots=2, n_coders=2)
out = {"which": args.label, "size": f"{H}x{W}", "repeats": args.repeats}
img = syn1(H, W, 1)
for near, effort in [(0, 2), (2, 2), (0, 3), (2, 3)]:
    ctx.encode_modes([img[:64, :64].copy()], [near], [effort])                # warm-up: code load, allocations
    s, _ = ctx.encode_modes([img], [near], [effort])
    ctx.decode_batch(s)
    enc, dec = [], []
    for r in range(args.repeats):
        t = time.perf_counter(); s, _ = ctx.encode_modes([img], [near], [effort]); enc.append((time.perf_counter() - t) * 1e6 / (H * W))
        t = time.perf_counter(); d = ctx.decode_batch(s); dec.append((time.perf_counter() - t) * 1e6 / (H * W))
        assert d[0] is not None
    out[f"n{near}_e{effort}"] = {"encode_us_per_px": [round(x, 4) for x in enc], "encode_median": round(float(np.median(enc)), 4),
                                 "decode_us_per_px": [round(x, 4) for x in dec], "decode_median": round(float(np.median(dec)), 4)}
ctx.close()
print(json.dumps(out))
