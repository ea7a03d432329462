"""Same-box A/B of the existing decoders: decode_batch of N x 512^2 SYN-1 frames per (codec, near, effort) class, best of
three calls.  The library under test is whichever libnblic_amd.so NBLIC_AMD_LIB names (default: the in-tree build), so
two builds are compared by running this twice, alternately, on one box.  Prints one JSON line.

    NBLIC_AMD_LIB=/path/to/other/libnblic_amd.so python tools/decode_ab.py --images 256
"""
import argparse, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=256)
ap.add_argument("--size", type=int, default=512)
args = ap.parse_args()
pkg = importlib.import_module("nblic-image-compression_amd")
ctx = pkg.Context(device=0, n_slots=24, n_coders=4, n_groups=2, n_host_buffers=48)
imgs = [pkg.syn1(args.size, args.size, 1 + k) for k in range(args.images)]
line = {"lib": os.environ.get("NBLIC_AMD_LIB", "in-tree"), "images": args.images, "size": args.size}
for near, effort in ((0, 1), (2, 1), (0, 2), (0, 3), (2, 2), (0, 0)):
    if effort == 0:
        streams = ctx.qencode_batch(imgs)
    else:
        streams, _ = ctx.encode_modes(imgs, [near] * len(imgs), [effort] * len(imgs), want_recon=False)
    best, ok = 1e9, True
    for _ in range(3):
        t0 = time.perf_counter()
        dec = ctx.decode_batch(streams)
        best = min(best, time.perf_counter() - t0)
        ok = ok and all(d is not None for d in dec)
    if effort == 0 or near == 0:
        ok = ok and all(np.array_equal(d[0], i) for d, i in zip(dec, imgs))
    line[f"n{near}_e{effort}" if effort else "qnblic"] = {"seconds": round(best, 4), "Mpixel_per_s": round(args.images * args.size ** 2 / best / 1e6, 2), "ok": bool(ok)}
ctx.close()
print(json.dumps(line), flush=True)
