"""Same-box A/B of the band decoder against the indexed decode (seek index, Context.decode_indexed: the indexed batch
decode with one image) on one large image per case.  Per case: the band decoder (decompress_bands), build_index, decode_indexed (best of --repeat calls), a
row-range decode of R rows from the middle, the segment count and index bytes / stream bytes.  Every plane is checked
bit-exact against the input (lossless).  Writes one JSON document.

    python tools/index_ab.py --out profiles/r06_indexed_decode.json
"""
import argparse, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--quick", action="store_true", help="small images (a check of the tool, not a measurement)")
args = ap.parse_args()
pkg = importlib.import_module("nblic-image-compression_amd")
ctx = pkg.Context(device=0, n_slots=2, n_coders=2)
# (h, w, effort, spacings R)
cases = [(4096, 4096, 1, (64, 256)), (1024, 2048, 3, (128,))]
if args.quick:
    cases = [(256, 256, 1, (16, 64)), (64, 128, 3, (16,))]


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t0


doc = {"what": "band decoder (decompress_bands, one wave) against the indexed decode (decode_indexed: one wave per segment, "
               "one launch set) on the same stream, same box, same process; SYN-1 images, -n0, planes checked bit-exact",
       "lib": os.environ.get("NBLIC_AMD_LIB", "in-tree"), "cases": []}
for h, w, effort, spacings in cases:
    img = pkg.syn1(h, w, 1)
    streams, _ = ctx.encode_modes([img], [0], [effort], want_recon=False)
    s = streams[0]
    band, t_band = timed(lambda: pkg.decompress_bands(s, ctx=ctx))
    assert np.array_equal(band, img)
    for R in spacings:
        ix, t_build = timed(lambda: ctx.build_index(s, R))
        best = 1e9
        for _ in range(args.repeat):
            plane, t = timed(lambda: ctx.decode_indexed(s, ix))
            assert np.array_equal(plane, img)
            best = min(best, t)
        r0 = (h // 2 // R) * R + R // 2
        rows, t_rows = timed(lambda: ctx.decode_rows(s, ix, r0, r0 + R))
        assert np.array_equal(rows, img[r0:r0 + R])
        case = {"h": h, "w": w, "near": 0, "effort": effort, "every_rows": R, "segments": (h - 1) // R + 1,
                "stream_bytes": len(s), "index_bytes": len(ix), "index_over_stream": round(len(ix) / len(s), 3),
                "band_decoder_s": round(t_band, 4), "build_index_s": round(t_build, 4), "decode_indexed_s": round(best, 4),
                "speedup": round(t_band / best, 2), "decode_rows_s": round(t_rows, 4), "decode_rows_range": [r0, r0 + R],
                "bit_exact": True}
        print(json.dumps(case), flush=True)
        doc["cases"].append(case)
ctx.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
