"""Which regimes of the chain kernels the images of the stage-level GPU tests reach (CPU only, oracle.stages): context chain
lengths against the 4096-record block and its 3072-record warm-up, which blocks' warm-up copies meet, where counter chains
start and end in their 512-touch windows, where halvings fall, and how many busy chains a touch segment has.  The families
of tests/chain_inputs.py are listed after them.

    python tools/chain_coverage.py
"""
import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import chain_inputs as ci      # noqa: E402
import inputs                  # noqa: E402
from oracle.oracle import Oracle      # noqa: E402


def seg_len(n_ev):             # kernels_e1.hip make_plan(n_ev, kTouchSegments)
    return (max(-(-n_ev // 256), 1024) + 63) & ~63


def model_row(fams):
    near, pattern, later, sandwiched = Counter(), Counter(), 0, 0
    for fam in fams:
        r = ci.ctx_replay(fam)
        for n in np.bincount(fam["adr"].astype(np.int64)):
            for edge in (4096, 7168):
                if abs(int(n) - edge) <= 1:
                    near[int(n)] += 1
        by_key = {}
        for k, b, met, *_ in r["blocks"]:
            by_key.setdefault(k, []).append(met)
        for mets in by_key.values():
            later += len(mets) - 1
            pattern.update(mets[1:])
            sandwiched += sum(1 for j in range(2, len(mets) - 1) if mets[j] and not mets[j - 1] and not mets[j + 1])
    return (f"chains of 4095/4096/4097/7167/7168/7169 records: {[near.get(n, 0) for n in (4095, 4096, 4097, 7167, 7168, 7169)]}; blocks behind a chain's first: "
            f"{later} (met {pattern.get(True, 0)}, not met {pattern.get(False, 0)}); met between two unmet: {sandwiched}")


def back_row(evs, seg=None):
    align, cut_first, cut_last, extra, per_window, lanes, slots, busy = Counter(), 0, 0, 0, Counter(), Counter(), set(), Counter()
    for ev in evs:
        counts, starts = ci.chain_layout(ev)
        for k in np.flatnonzero(counts):
            p, n = int(starts[k] & 7), int(counts[k])
            align[p] += 1
            cut_last += (p + n) % 512 in (0, 1, 511)
            cut_first += n <= 9 - p
            extra += (n - 1) // 512 + 1 < (p + n + 511) // 512
        pw, ln, sl = ci.halving_slots(ev)
        per_window.update(pw.values())
        lanes.update(l for l in ln if l in (0, 63))
        slots |= sl
        a, b, _ = ci.busy_chains(ev, seg or seg_len(len(ev)))
        busy.update(int(v) for v in np.r_[a, b])
    edge = {n: busy.get(n, 0) for n in (63, 64, 65)}
    return (f"chain starts & 7 seen: {sorted(align)}; chains ending within a slot of a window edge: {cut_last}, of at most 9 - p touches: {cut_first}, "
            f"with the extra window: {extra}; halvings per window: {dict(sorted(per_window.items()))}; halvings in lane 0 / 63: {lanes.get(0, 0) > 0} / {lanes.get(63, 0) > 0}, "
            f"lane-local slots {sorted(slots)}; busy chains (>= 16 touches) per segment and parity: max {max(busy)}, exactly 63/64/65: {edge}")


def of_image(o, img):
    st = o.stages(img)
    fam = dict(model=0, adr=st["adr"], px0=st["px0"], x=np.ascontiguousarray(img).reshape(-1))
    ev = ci.pack_event(st["cu"] >> 8, st["cv"] >> 8, st["cu"] & 255, st["ev_qw"], st["ev_bin"])
    return fam, ev


def main():
    o = Oracle()
    _, arrays = inputs.fixtures()
    crops = [np.ascontiguousarray(c) for c in arrays["kodak_crops"]]
    half = inputs.make("const", 200, 300).copy()
    half[:, 150:] = inputs.make("noise", 200, 150)
    bands = inputs.make("ramp", 256, 256).copy()
    bands[64:192] = 200
    groups = {
        "test_stage_parity": [inputs.make(c, h, w) for (h, w) in [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (17, 13), (40, 37), (64, 64), (96, 128), (5, 300)]
                              for c in ("syn1", "noise", "checker", "const", "ramp")],
        "test_stage_parity_photographic": [crops[4], np.ascontiguousarray(np.block([[crops[4 * r + c] for c in range(4)] for r in range(4)]))],
        "test_flat_and_structured_images_multi_block": [inputs.make("const", 200, 300), inputs.make("ramp", 256, 256), inputs.make("checker", 300, 300), half, bands,
                                                        np.zeros((130, 1000), np.uint8), np.full((500, 90), 255, np.uint8)],
    }
    for name, imgs in groups.items():
        both = [of_image(o, img) for img in imgs]
        print(f"{name} ({len(imgs)} images)\n  model: {model_row([b[0] for b in both])}\n  back:  {back_row([b[1] for b in both])}")
    for model in (0, 1):
        print(f"chain_inputs model {model}\n  model: {model_row(list(ci.model_families(model).values()))}")
    print(f"chain_inputs back half\n  back:  {back_row(list(ci.back_families().values()))}")
    print(f"chain_inputs staging_wide\n  back:  {back_row([ci.staging_wide_family()], ci.WIDE_SEG)}")


if __name__ == "__main__":
    main()
