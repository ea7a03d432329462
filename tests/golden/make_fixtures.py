"""Regenerates tests/golden/reference_fixtures.{npz,json}: what the compiled, unmodified reference (oracle/_ref) and its
Kodak images give, kept small so that the tests that compare against the reference run without the reference tree.

Runs only where `oracle.build()` compiled oracle/_ref from the reference sources (and the Kodak BMPs are readable).
Contains no reference code: it calls the reference's compiled libraries through ctypes and reads `nm` output.
  reference_fixtures.npz
    kodak_crops         uint8 [24, 64, 96]   inputs.KODAK_CROP of every Kodak image (the images' own pixels)
    kodak_bmp_headers   uint8 [24, 1078]     each Kodak BMP's file header, info header and palette
    fileio_<fmt>_<h>x<w>  uint8              the bytes the reference's writer puts in a file for inputs.make("noise", h, w)
    case_<k>, q_case_<k>  uint8              the reference's streams of inputs.random_cases() / inputs.random_q_cases()
  reference_fixtures.json
    kodak_crops         name -> -e1 and -e0 stream length + SHA-256 of the crop
    case_recon_sha256   the reference's decode of case_<k> (SHA-256 of the plane)
    main_codec_symbols  the codec symbols the reference's command-line caller (NBLIC_main.c) needs from a library
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import inputs  # noqa: E402
from oracle.oracle import Reference  # noqa: E402

FILEIO_SHAPES = [(1, 1), (3, 5), (17, 13), (64, 61), (30, 128)]


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def fileio_bytes(tmp):
    import ctypes as C
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libfileio_ref.so"))
    u8p = C.POINTER(C.c_uint8)
    out = {}
    for (h, w) in FILEIO_SHAPES:
        img = inputs.make("noise", h, w)
        for fmt, writer in (("pgm", lib.writePGMImageFile), ("bmp", lib.writeBMPGrayImageFile)):
            path = os.path.join(tmp, f"{fmt}_{h}x{w}")
            assert writer(path.encode(), img.ctypes.data_as(u8p), h, w) == 0
            out[f"fileio_{fmt}_{h}x{w}"] = np.frombuffer(open(path, "rb").read(), np.uint8)
    return out


def main_codec_symbols():
    def names(args):
        r = subprocess.run(["nm"] + args, capture_output=True, text=True, check=True)
        return {l.split()[-1] for l in r.stdout.splitlines() if l.strip()}
    ref = os.path.join(ROOT, "oracle", "_ref")
    needed = names(["-u", os.path.join(ref, "NBLIC_main.o")]) - names(["--defined-only", os.path.join(ref, "FileIO.o")])
    return sorted(needed & names(["-D", "--defined-only", os.path.join(ref, "libnblic_ref.so")]))


def main():
    import tempfile
    ref = Reference()
    arrays, meta = {}, {"kodak_crops": {}, "case_recon_sha256": [], "main_codec_symbols": main_codec_symbols()}
    names = sorted(os.listdir(inputs.KODAK_DIR))
    crops, headers = [], []
    for name in names:
        path = os.path.join(inputs.KODAK_DIR, name)
        crop = np.ascontiguousarray(inputs.read_gray_bmp(path)[inputs.KODAK_CROP])
        crops.append(crop)
        headers.append(np.frombuffer(open(path, "rb").read(1078), np.uint8))
        s, q = ref.encode(crop, 0, 1)[0], ref.qencode(crop)
        meta["kodak_crops"][name] = {"len": len(s), "sha256": sha(s), "q_len": len(q), "q_sha256": sha(q)}
    arrays["kodak_crops"] = np.stack(crops)
    arrays["kodak_bmp_headers"] = np.stack(headers)
    with tempfile.TemporaryDirectory() as tmp:
        arrays.update(fileio_bytes(tmp))
    for k, (img, near, effort) in enumerate(inputs.random_cases()):
        s = ref.encode(img, near, effort)[0]
        arrays[f"case_{k}"] = np.frombuffer(s, np.uint8)
        meta["case_recon_sha256"].append(sha(ref.decode(s)[0].tobytes()))
    for k, img in enumerate(inputs.random_q_cases()):
        arrays[f"q_case_{k}"] = np.frombuffer(ref.qencode(img), np.uint8)
    np.savez_compressed(os.path.join(HERE, "reference_fixtures.npz"), **arrays)
    with open(os.path.join(HERE, "reference_fixtures.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
