"""Deterministic synthetic gray planes shared by the fixture generator and the tests.

Pure integer numpy, no RNG state, so the same bytes come out on every machine.
"""
import numpy as np

SMALL_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3), (17, 13), (64, 64), (256, 2), (2, 256)]
CONTENTS = ["const", "ramp", "checker", "noise", "syn1"]
# (near, effort) classes of SURVEY.md section 8c; effort 0 / near 12 exercise the clamps
PARAM_CLASSES = [(0, 1), (0, 2), (0, 3), (1, 1), (2, 1), (2, 2), (9, 1), (3, 3), (12, 0)]


def syn1(h, w, seed=1):
    """SYN-1: xorshift32 noise on a triangular ramp with a 16-level texture."""
    n = h * w
    xs = np.empty(n, np.uint32)
    s = seed & 0xFFFFFFFF
    # the xorshift chain is serial; do it in python for small frames, in blocks otherwise
    for k in range(n):
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        xs[k] = s
    xs = xs.reshape(h, w)
    i = np.arange(h, dtype=np.int64)[:, None]
    j = np.arange(w, dtype=np.int64)[None, :]
    t = ((i + 2 * j) >> 3) & 511
    base = np.minimum(255, np.abs(t - 256))
    tex = (i ^ j) & 15
    noise = (xs & 7).astype(np.int64) + ((xs >> 3) & 7).astype(np.int64) - 7
    return np.clip(((base * 3) >> 2) + 32 + tex + noise, 0, 255).astype(np.uint8)


def noise(h, w, seed=7):
    idx = np.arange(h * w, dtype=np.uint64) + np.uint64(seed) * np.uint64(1000003)
    v = idx * np.uint64(0x9E3779B97F4A7C15)
    v ^= v >> np.uint64(29)
    v *= np.uint64(0xBF58476D1CE4E5B9)
    v ^= v >> np.uint64(32)
    return (v & np.uint64(255)).astype(np.uint8).reshape(h, w)


def make(content, h, w):
    if content == "const":
        return np.full((h, w), 77, np.uint8)
    if content == "ramp":
        return ((np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 5) % 256).astype(np.uint8)
    if content == "checker":
        return (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)
    if content == "noise":
        return noise(h, w)
    if content == "syn1":
        return syn1(h, w)
    raise ValueError(content)


# Hard-edged planes (two levels, 0 and 255: text scans, charts, screenshots).  Coded near-lossless at efforts 2 / 3 they
# push the least-squares systems out of the range in which the kernels' doubles are exact, so pixels are redone with
# 64-bit integers (csrc/lsq_f64.h Guard) -- which CONTENTS practically never does.  Not part of CONTENTS: the golden
# streams are made from that list.
HARD_EDGED = ["step_v", "step_h", "stripes_h", "bars_v"]


def blocks(h, w, block, seed):
    """Random 0 / 255 squares of side `block` (xorshift32, one draw per square)."""
    gh, gw = -(-h // block), -(-w // block)
    bits = np.empty(gh * gw, np.uint8)
    s = (seed * 2654435761 + 1) & 0xFFFFFFFF
    for k in range(gh * gw):
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        bits[k] = (s >> 7) & 1
    grid = bits.reshape(gh, gw) * np.uint8(255)
    return np.ascontiguousarray(np.repeat(np.repeat(grid, block, 0), block, 1)[:h, :w])


def make_hard(content, h, w):
    if content == "step_v":                       # left half 0, right half 255
        return np.ascontiguousarray(np.broadcast_to(((np.arange(w) >= w // 2) * 255).astype(np.uint8)[None, :], (h, w)))
    if content == "step_h":                       # top half 0, bottom half 255
        return np.ascontiguousarray(np.broadcast_to(((np.arange(h) >= h // 2) * 255).astype(np.uint8)[:, None], (h, w)))
    if content == "stripes_h":                    # rows alternate 0 / 255
        return np.ascontiguousarray(np.broadcast_to(((np.arange(h) & 1) * 255).astype(np.uint8)[:, None], (h, w)))
    if content == "bars_v":                       # columns alternate 0 / 255 in bars of 64: an edge every 64 pixels of however wide a row
        return np.ascontiguousarray(np.broadcast_to((((np.arange(w) >> 6) & 1) * 255).astype(np.uint8)[None, :], (h, w)))
    if content == "blocks_lossless":              # the one of 60 block planes (block 1..16, 20..80 x 20..120) that reaches the redo LOSSLESS
        return blocks(33, 81, 13, 28)             # with several pixels (-e2: 4, -e3: 15); h and w are not used
    raise ValueError(content)


def spikes(h=32, w=48):
    """A flat plane (77) with isolated extremes: 255 on a 7 x 5 grid, 0 on an 11 x 9 grid.  In a quiet context every
    spike is a symbol of a hundred and more, so the binarisation's unary prefix runs far past 64 ones."""
    img = np.full((h, w), 77, np.uint8)
    img[::7, ::5] = 255
    img[3::11, 2::9] = 0
    return img


# Streams no encoder writes.  A decoder takes k_step from byte 14 of the header and accepts 3..16 with any near 0..9
# (NBLIC.c:733-745, :765); the encoders only ever write clip(3 + 2 near, 3, 16).  The 140 pairs, in the fixed order the
# hashes of tests/golden/foreign_streams.json are taken in:
FOREIGN_PAIRS = [(near, k_step) for near in range(10) for k_step in range(3, 17)]
FOREIGN_EFFORTS = (1, 2, 3)


def paired_k_step(near):
    return min(max(3 + 2 * near, 3), 16)


def foreign_planes():
    """name -> plane: the smallest planes that between them reach every regime of the binarisation walk at every k_step
    (test_oracle.py test_foreign_planes_reach_every_walk_regime); at most 2700 pixels each."""
    _, arrays = fixtures()
    return {
        "kodak05": np.ascontiguousarray(arrays["kodak_crops"][4][:40, :56]),
        "blocks": make_hard("blocks_lossless", 33, 81),
        "noise": noise(24, 40),
        "syn1": syn1(24, 40),
        "spikes": spikes(),
        "checker": make("checker", 17, 13),
    }


def foreign_streams(oracle, plane, efforts=FOREIGN_EFFORTS, pairs=None):
    """[((near, k_step, effort), stream, reconstruction)] from the oracle, efforts outermost, pairs in FOREIGN_PAIRS order."""
    out = []
    for effort in efforts:
        for near, k_step in (FOREIGN_PAIRS if pairs is None else pairs):
            s, rec, *_ = oracle.encode(plane, near, effort, k_step=k_step)
            out.append(((near, k_step, effort), s, rec))
    return out


def foreign_golden():
    """tests/golden/foreign_streams.json (make_foreign.py): per "<plane>_e<effort>" the SHA-256 of the 140 oracle streams
    concatenated and of the 140 planes the compiled reference decoded them to."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "foreign_streams.json")) as f:
        return json.load(f)


def case_id(content, h, w, near, effort):
    return f"{content}_{h}x{w}_n{near}_e{effort}"


def random_cases():
    """The oracle-vs-reference sample of test_oracle.py: (img, near, effort) on random shapes up to 47x47."""
    rng = np.random.default_rng(1234)
    out = []
    for _ in range(25):
        h, w = int(rng.integers(1, 48)), int(rng.integers(1, 48))
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        if rng.random() < 0.5:
            img = (img // 16 + make("ramp", h, w) // 2).astype(np.uint8)
        out.append((img, int(rng.integers(0, 10)), int(rng.integers(1, 4))))
    return out


def random_q_cases():
    """The effort-0 sample of test_oracle_q.py: random shapes up to 39x39 plus one 200x300 SYN-1 frame."""
    rng = np.random.default_rng(77)
    out = []
    for _ in range(30):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        if rng.random() < 0.6:
            img = (img // 32 + make("ramp", h, w) // 2 + 40).astype(np.uint8)
        out.append(img)
    return out + [syn1(200, 300, 4)]


KODAK_DIR = "/root/reference/img_kodak"      # read in place, container only; never copied into the repo
KODAK_CROP = (slice(192, 256), slice(320, 416))   # the 64x96 window of every Kodak image kept in tests/golden/reference_fixtures.npz


def fixtures():
    """tests/golden/reference_fixtures.{npz,json}: data the compiled reference produced (tests/golden/make_fixtures.py),
    so that the checks against it run without the reference tree."""
    import json
    import os
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(g, "reference_fixtures.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(g, "reference_fixtures.npz"), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    return meta, arrays


def read_gray_bmp(path):
    """8-bit palettised gray BMP as the reference's reader sees it (FileIO.c:170-287): bottom-up
    rows, 4-byte row padding, pixel = palette index (the Kodak files carry an identity palette)."""
    import struct
    raw = open(path, "rb").read()
    off = struct.unpack_from("<I", raw, 10)[0]
    w, h = struct.unpack_from("<ii", raw, 18)
    bpp = struct.unpack_from("<H", raw, 28)[0]
    assert bpp == 8 and raw[:2] == b"BM"
    stride = (w + 3) & ~3
    rows = np.frombuffer(raw, np.uint8, count=stride * abs(h), offset=off).reshape(abs(h), stride)[:, :w]
    return np.ascontiguousarray(rows[::-1] if h > 0 else rows)
