"""Regenerates tests/golden/foreign_q_streams.json: hashes of valid QNBLIC (effort 0) streams that no encoder writes, as
the compiled, unmodified reference (oracle/_ref) decodes them.

A QNBLIC stream carries its twelve frequency tables; every encoder writes the scaled true counts in the greedy histogram
code.  tests/q_foreign_inputs.py makes streams with other tables (fixed points of the scaling, handed to the oracle's
entropy stage) and other codes of the same tables (its re-coder).  The reference decodes each stream, and per
"<plane>/<family>" the file keeps
  streams_sha256   SHA-256 of the streams of q_foreign_inputs.POLICIES concatenated in that order
  planes_sha256    SHA-256 of the planes the reference decoded them to, concatenated in the same order
  bytes            total length of those streams
Runs only where `oracle.build()` compiled oracle/_ref from the reference sources.  Contains no reference code: it calls
the reference's compiled library through ctypes.  A stream the reference does not decode to the plane it was made from
stops the run.
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
import q_foreign_inputs as qf  # noqa: E402
from oracle.oracle import Oracle, Reference  # noqa: E402


def main():
    oracle, ref = Oracle(), Reference()
    meta = {}
    for c in qf.cases(oracle):
        d = ref.qdecode(c.stream)
        assert d is not None and np.array_equal(d, c.plane), (c.plane_name, c.family, c.policy)
        m = meta.setdefault(f"{c.plane_name}/{c.family}", {"s": hashlib.sha256(), "p": hashlib.sha256(), "bytes": 0, "policies": []})
        m["s"].update(c.stream)
        m["p"].update(d.tobytes())
        m["bytes"] += len(c.stream)
        m["policies"].append(c.policy)
    assert all(m["policies"] == list(qf.POLICIES) for m in meta.values())
    out = {k: {"streams_sha256": m["s"].hexdigest(), "planes_sha256": m["p"].hexdigest(), "bytes": m["bytes"]} for k, m in meta.items()}
    with open(os.path.join(HERE, "foreign_q_streams.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
