"""Regenerates tests/golden/foreign_streams.json: hashes of valid streams that no encoder writes, as the compiled,
unmodified reference (oracle/_ref) decodes them.

A decoder takes k_step from the stream header and accepts any 3..16 with any near 0..9; every encoder writes
clip(3 + 2 near, 3, 16).  The oracle codes each plane of inputs.foreign_planes() with all 140 (near, k_step) pairs at
every effort (Oracle.encode(..., k_step=)), the reference decodes each stream, and per "<plane>_e<effort>" the file keeps
  streams_sha256   SHA-256 of the 140 oracle streams concatenated in inputs.FOREIGN_PAIRS order
  planes_sha256    SHA-256 of the 140 planes the reference decoded them to, concatenated in the same order
  bytes            total length of the 140 streams
Runs only where `oracle.build()` compiled oracle/_ref from the reference sources.  Contains no reference code: it calls
the reference's compiled library through ctypes.  A stream the reference does not decode to the oracle's reconstruction,
or farther than near from the plane, stops the run.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import inputs  # noqa: E402
from oracle.oracle import Oracle, Reference  # noqa: E402


def main():
    oracle, ref = Oracle(), Reference()
    meta = {}
    for name, plane in inputs.foreign_planes().items():
        for effort in inputs.FOREIGN_EFFORTS:
            hs, hp, total = hashlib.sha256(), hashlib.sha256(), 0
            for (near, k_step, _), s, rec in inputs.foreign_streams(oracle, plane, (effort,)):
                d = ref.decode(s)
                assert d is not None and d[1:] == (near, effort), (name, near, k_step, effort)
                assert np.array_equal(d[0], rec), (name, near, k_step, effort)
                assert int(np.abs(d[0].astype(int) - plane.astype(int)).max()) <= near, (name, near, k_step, effort)
                hs.update(s)
                hp.update(d[0].tobytes())
                total += len(s)
            meta[f"{name}_e{effort}"] = {"streams_sha256": hs.hexdigest(), "planes_sha256": hp.hexdigest(), "bytes": total}
    with open(os.path.join(HERE, "foreign_streams.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
