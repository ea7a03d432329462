"""Frames for the colour plan's tests (tests/test_color_plan_host.py on the CPU, tests/test_color_plan_kernels.py and
tests/test_color_modes_codec.py on the GPU): cost tasks at the smallest shapes at which the tile walk can go wrong, as the
dicts that ``Context.debug_color_cost`` takes -- plus, per task, the collected planes the numpy restatement needs -- and the
four constructed classes of frames whose modes the rule must find."""
import numpy as np

import inputs
from collect_inputs import ELEM, NORMS, as_values, element_bits, lay_out
from rct_inputs import exhaustive_frame

TILE = 64                                                      # cost_tile.h kCostTile
# a pixel, one row, one column, a few of each; one tile exactly; a row and a column more; two tiles each way plus one
SHAPES = ((1, 1), (1, 17), (17, 1), (3, 5), (TILE, TILE), (TILE + 1, TILE + 1), (2 * TILE + 1, 2 * TILE + 1),
          (TILE + 1, 2 * TILE + 2), (2 * TILE + 2, TILE + 1))       # (2 x 3 and 3 x 2 tiles: a grid that is not square)
LAYOUTS = ("contiguous", "interleaved", "pitched")


def _source(bits, fmt, layout, k, ch):
    """(raw bytes, pitch, step) of one channel: contiguous; every third element as in an interleaved RGB row; or
    contiguous rows with slack behind them, another for every channel."""
    rows, cols = bits.shape
    e = ELEM[fmt]
    if layout == "contiguous":
        pitch, step = cols * e, e
    elif layout == "interleaved":
        pitch, step = cols * 3 * e, 3 * e
    else:
        pitch, step = (cols + 1 + (k + ch) % 3) * e, e
    return lay_out(bits, fmt, pitch, step, 0), pitch, step


def cost_tasks(pkg, seed=26):
    """Every shape in every format and layout, with a scale and bias from collect_inputs.NORMS, at odd base offsets, and
    the exhaustive frame.  Each task carries ``planes``: the three collected uint8 planes by ``collect_numpy``."""
    rng = np.random.default_rng(seed)
    tasks, k = [], 0
    for fmt in range(4):
        e = ELEM[fmt]
        for rows, cols in SHAPES:
            for layout in LAYOUTS:
                scale, bias = NORMS[0] if fmt == 0 else NORMS[k % 3]
                bits = [element_bits(rng, fmt, (rows, cols)) for _ in range(3)]
                laid = [_source(bits[ch], fmt, layout, k, ch) for ch in range(3)]
                tasks.append(dict(raws=[l[0] for l in laid], pitches=[l[1] for l in laid], steps=[l[2] for l in laid], rows=rows, cols=cols, fmt=fmt,
                                  scale=scale, bias=bias, base_offsets=[((2 * k + 1 + 2 * ch) * e) % 256 for ch in range(3)], layout=layout,
                                  planes=[pkg.collect_numpy(as_values(b, fmt), fmt, scale, bias) for b in bits]))
                k += 1
    r, g, b = exhaustive_frame()
    tasks.append(dict(raws=[r.copy(), g.copy(), b.copy()], pitches=[256] * 3, steps=[1] * 3, rows=256, cols=256, fmt=0, scale=1.0, bias=0.0,
                      base_offsets=[0, 3, 5], layout="contiguous", planes=[r, g, b]))
    return tasks


def mix(a, b):
    return ((7 * a.astype(np.uint16) + b) // 8).astype(np.uint8)


CLASSES = ("shared", "independent", "r and b shared", "equal")


def class_frames(h, w, seed=40):
    """[4, 3, h, w] uint8, one frame per class of CLASSES: three channels that share a SYN-1 plane (7 parts in 8, the
    eighth a plane of the channel's own seed); three planes of independent seeds; R and B share a plane and G is
    independent; R = G = B."""
    s = lambda k: inputs.syn1(h, w, seed + k)
    shared = np.stack([mix(s(0), s(1 + c)) for c in range(3)])
    independent = np.stack([s(4 + c) for c in range(3)])
    rb = np.stack([mix(s(7), s(8)), s(9), mix(s(7), s(10))])
    equal = np.stack([s(11)] * 3)
    return np.stack([shared, independent, rb, equal])


def check_class_modes(pkg, modes, costs=None):
    """What the rule must make of class_frames: both differences (the base is whichever total is smallest: the three lie
    within 0.3 % of each other); plain; base R or B with exactly the other of the two as a difference and G plain; 0x0D."""
    m = [int(v) for v in modes]
    assert m[0] & 12 == 12, m
    assert m[1] == 0, m
    assert m[2] in (0x08, 0x04 | 2), m                          # base R: B is its higher-numbered other; base B: R is its lower-numbered other
    assert m[3] == pkg.COLOR_RCT, m
