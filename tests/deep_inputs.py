"""Deep (16-bit) images for the deep-pixel tests (tests/test_deep_host.py on the CPU, tests/test_deep_kernels.py and
tests/test_deep_codec.py on the GPU): the shapes, layouts and values at which the unit and tile walks can go wrong, the
tasks as ``Context.debug_deep_collect`` / ``debug_deep_deliver`` / ``debug_deep_cost`` take them, numpy restatements of
what each must produce, written independently of csrc/deep.h, and the constructed classes whose modes the rule must find.
Everything here is CONSTRUCTED: no real radiograph or CT slice is at hand."""
import numpy as np

import inputs

PATTERN = 0x5A                                                   # what every output buffer holds before a walk or a launch
GUARD = 256                                                      # bytes of it around a collected plane on the device
# a pixel; one row with a unit and a pixel; fewer pixels than a unit; a unit and a tile edge on both sides; one tile
# exactly; a row and two columns more than a tile, two units and two more than eight
SHAPES = ((1, 1), (1, 17), (3, 5), (33, 65), (64, 64), (65, 130), (130, 65))   # (the last two: 2 x 3 and 3 x 2 tiles)
LAYOUTS = ("contiguous", "pitched", "step 6", "odd offset")
EDGE_U = (0, 255, 256, 257, 0x7FFF, 0x8000, 0xFFFF)               # u at the byte and the sign boundaries
EDGE_I16 = (-32768, -1, 0)
ELEM = (2, 2, 2, 2, 4)                                           # bytes of a destination element, by deep destination format
BITLEN = np.array([int(v).bit_length() for v in range(256)], np.int64)


def random_image(rng, h, w, signed=False):
    """h x w of 16-bit values: a smooth ramp with noise that crosses many high-byte steps, the edge values sprinkled in."""
    yy, xx = np.mgrid[0:h, 0:w]
    u = (20000 + 37 * xx + 91 * yy + rng.integers(-300, 300, (h, w))) & 0xFFFF
    flat = u.reshape(-1)
    at = rng.permutation(flat.size)[:len(EDGE_U)]
    flat[at] = EDGE_U[:len(at)]
    u = u.astype(np.uint16)
    return (u ^ np.uint16(0x8000)).view(np.int16) if signed else u


def unsigned_of(x):
    """u of an array of uint16 or int16 elements: int64."""
    x = np.asarray(x)
    return x.astype(np.int64) + (32768 if x.dtype == np.int16 else 0)


def planes_numpy(x, fold):
    """(high, low) uint8 of a 16-bit array, by arithmetic on wide integers."""
    u = unsigned_of(x)
    hi, lo = u // 256, u % 256
    if fold:
        lo = np.where(hi % 2 == 1, 255 - lo, lo)
    return hi.astype(np.uint8), lo.astype(np.uint8)


def part_numpy(x, part):
    return planes_numpy(x, part == 2)[0 if part == 0 else 1]


def plane_cost_numpy(p):
    """The cost of one uint8 plane: MED prediction (row 0: W; column 0: N; (0, 0): 128), e = p - pred NOT wrapped, the sum
    of 2 * bitlen(|e|) + 1."""
    p = p.astype(np.int64)
    pred = np.empty_like(p)
    pred[0, 0] = 128
    pred[0, 1:] = p[0, :-1]
    pred[1:, 0] = p[:-1, 0]
    w, n, nw = p[1:, :-1], p[:-1, 1:], p[:-1, :-1]
    pred[1:, 1:] = np.where(nw >= np.maximum(w, n), np.minimum(w, n), np.where(nw <= np.minimum(w, n), np.maximum(w, n), w + n - nw))
    return int((2 * BITLEN[np.abs(p - pred)] + 1).sum())


def sums_numpy(x):
    """What the cost walk reports for an image: the costs of the high, the low and the folded low plane, min and max of u."""
    u = unsigned_of(x)
    return np.array([plane_cost_numpy(part_numpy(x, k)) for k in range(3)] + [int(u.min()), int(u.max())], np.uint64)


def lay_out(x, layout, rng):
    """A 16-bit image as raw bytes in one of the LAYOUTS: (bytes, offset, pitch, step), every byte that is no element 0xFF."""
    h, w = x.shape
    step = 6 if layout == "step 6" else 2
    pitch = w * step + (0 if layout == "contiguous" else 2 * int(rng.integers(1, 9)))
    offset = 2 * int(rng.integers(0, 8)) + 1 if layout == "odd offset" else 0      # an odd number of 2-byte elements into the region
    offset *= 2 if layout == "odd offset" else 1
    raw = np.full(offset + (h - 1) * pitch + (w - 1) * step + 2 + 14, 0xFF, np.uint8)
    src = np.ascontiguousarray(x).view(np.uint8).reshape(h, w, 2)
    rows, cols = np.mgrid[0:h, 0:w]
    at = offset + rows * pitch + cols * step
    raw[at] = src[..., 0]
    raw[at + 1] = src[..., 1]
    return raw, offset, pitch, step


def collect_tasks(seed=5):
    """One task per shape, layout, source format and part, the shapes' pixel ranges varied, and one larger than a chunk."""
    rng = np.random.default_rng(seed)
    tasks = []
    k = 0
    for h, w in SHAPES + ((130, 130),):                        # (130 x 130 = 16900 pixels: 1057 units, two chunks)
        for layout in LAYOUTS:
            signed = k % 2 == 1
            x = random_image(rng, h, w, signed)
            raw, offset, pitch, step = lay_out(x, layout, rng)
            t = dict(raw=raw[offset:], image=x, rows=h, cols=w, fmt=int(signed), part=k % 3, pitch=pitch, step=step,
                     base_offset=(2 * (k % 5) + (2 if layout == "odd offset" else 0)), full=raw, offset=offset)
            if k % 4 == 3 and h * w > 40:                      # a range with a short first and a short last unit
                t["px_range"] = (5, h * w - 3)
            tasks.append(t)
            k += 1
    return tasks


def expected_plane(t):
    """The plane a collect task leaves: the part's bytes inside its pixel range, the pattern elsewhere."""
    want = part_numpy(t["image"], t["part"]).reshape(-1).copy()
    p0, p1 = t.get("px_range", (0, want.size))
    keep = np.zeros(want.size, bool)
    keep[p0:p1 or want.size] = True
    return np.where(keep, want, PATTERN).astype(np.uint8).reshape(t["rows"], t["cols"])


def value_bits(u, mode, fmt, scale, bias):
    """The destination elements of u (int64) as unsigned integers, by numpy: the value, or float(v) * scale + bias in
    float32 -- two roundings -- rounded to nearest even into the format."""
    v = u - 32768 if mode & 2 else u
    if fmt == 0:
        return u.astype(np.uint32)
    if fmt == 1:
        return (u - 32768).astype(np.int16).view(np.uint16).astype(np.uint32)
    with np.errstate(all="ignore"):
        f = v.astype(np.float32) * np.float32(scale)
        f = f + np.float32(bias)
        if fmt == 4:
            return f.view(np.uint32)
        if fmt == 2:
            return f.astype(np.float16).view(np.uint16).astype(np.uint32)
    b = f.view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint32)


def expected_buffer(t):
    """What a deliver task's buffer holds afterwards, by numpy: the joined window scattered into a buffer of the pattern;
    zeros in the window when the task's zero flag is set or a gate is not done."""
    r0, r1, c0, c1 = t["window"]
    fmt, mode, elem = t["fmt"], t["mode"], ELEM[t["fmt"]]
    hi, lo = t["hi"].astype(np.int64), t["lo"].astype(np.int64)
    if mode & 1:
        lo = np.where(hi % 2 == 1, 255 - lo, lo)
    bits = value_bits((hi * 256 + lo)[r0:r1, c0:c1], mode, fmt, t.get("scale", 1.0), t.get("bias", 0.0))
    if t.get("zero") or any(g not in (-1, 1) for g in t.get("gate_status", (-1, -1))):
        bits = np.zeros_like(bits)
    step = t.get("step", elem)
    pitch = t.get("pitch", (c1 - c0) * step)
    off = t.get("offset", 0)
    size = t.get("out_bytes", off + (r1 - r0 - 1) * pitch + (c1 - c0 - 1) * step + elem)
    out = np.full(size, PATTERN, np.uint8)
    rows, cols = np.mgrid[0:r1 - r0, 0:c1 - c0]
    at = off + rows * pitch + cols * step
    for b in range(elem):
        out[at + b] = (bits >> (8 * b)) & 0xFF
    return out


def deliver_tasks(seed=6):
    """Windows with a head and a tail, destinations at 2 mod 16 bytes, pitched, strided and transposed destinations, every
    format and mode that go together, a gate that is not done, a zero flag, guard bytes around every window, and one task
    larger than a chunk."""
    rng = np.random.default_rng(seed)
    tasks = []
    k = 0
    for h, w in SHAPES + ((262, 72),):                         # (a window of 260 x 70 uint16: five units a row, 1300 units, two chunks)
        for kind in ("whole", "window", "strided", "transposed"):
            fmt = k % 5
            mode = (k // 5) % 4
            if fmt == 0:
                mode &= 1
            if fmt == 1:
                mode |= 2
            x = random_image(rng, h, w, bool(mode & 2))
            hi, lo = planes_numpy(x, mode & 1)
            elem = ELEM[fmt]
            win = (0, h, 0, w) if kind == "whole" or h < 3 or w < 3 else (1, h - 1, 1, w - 1)
            rows, cols = win[1] - win[0], win[3] - win[2]
            t = dict(hi=hi, lo=lo, window=win, fmt=fmt, mode=mode, base_offsets=(k % 16, (3 * k + 1) % 16))
            if fmt >= 2:
                t["scale"], t["bias"] = (1.0, 0.0) if k % 3 == 0 else (1.0 / 257.0, -3.5)
            if kind == "strided":
                t["step"] = 3 * elem
                t["pitch"] = cols * t["step"] + 2 * elem
            elif kind == "transposed":                         # element (r, c) at c * rows + r: a step larger than the pitch
                t["step"] = (rows + 1) * elem
                t["pitch"] = elem
            elif kind == "window":
                t["pitch"] = cols * elem + 6 * elem
            step = t.get("step", elem)
            pitch = t.get("pitch", cols * step)
            t["offset"] = 16 + (2 if fmt != 4 else 4) * (1 + k % 3) if kind != "whole" else 32      # 2 mod 16 and its kin; a whole image on a block
            t["out_bytes"] = t["offset"] + (rows - 1) * pitch + (cols - 1) * step + elem + 24
            if k % 7 == 5:
                t["gate_status"] = (1, 3) if k % 2 else (0, 1)
            elif k % 7 == 6:
                t["gate_status"] = (1, 1)
            if k % 11 == 10:
                t["zero"] = True
            tasks.append(t)
            k += 1
    return tasks


def cost_tasks(seed=7):
    rng = np.random.default_rng(seed)
    tasks = []
    k = 0
    for h, w in SHAPES + ((129, 70),):
        for layout in LAYOUTS:
            x = random_image(rng, h, w, k % 2 == 1)
            raw, offset, pitch, step = lay_out(x, layout, rng)
            tasks.append(dict(raw=raw[offset:], image=x, rows=h, cols=w, fmt=k % 2, pitch=pitch, step=step,
                              base_offset=(2 * (k % 7) + (2 if layout == "odd offset" else 0)), full=raw, offset=offset))
            k += 1
    return tasks


# ---- the constructed classes ------------------------------------------------------------------------------------------------------
def smooth_field(h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return 1800 + 1500 * np.sin(xx / 37) * np.cos(yy / 53) + 1.5 * (xx + yy)


def _noisy(base, sigma, top, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(base + rng.normal(0, sigma, base.shape)), 0, top).astype(np.uint16)


def class_image(name, h=256, w=256, seed=0, syn1=inputs.syn1):
    """One uint16 image of a class; ``seed`` varies the noise and the SYN-1 plane (``syn1``: who makes that plane)."""
    f = smooth_field(h, w)
    syn = syn1(h, w, 11 + seed).astype(np.float64) if "SYN-1" in name else None
    if name == "smooth 12-bit + N(0, 2)":
        return _noisy(np.clip(f, 0, 4095), 2, 4095, 101 + seed)
    if name == "smooth 12-bit + N(0, 8)":
        return _noisy(np.clip(f, 0, 4095), 8, 4095, 102 + seed)
    if name == "smooth 12-bit + N(0, 40)":
        return _noisy(np.clip(f, 0, 4095), 40, 4095, 103 + seed)
    if name == "SYN-1 x 16 + N(0, 4)":
        return _noisy(syn * 16, 4, 65535, 104 + seed)
    if name == "smooth x 16 + N(0, 30)":
        return _noisy(np.clip(f, 0, 4095) * 16, 30, 65535, 105 + seed)
    if name == "SYN-1 x 257":
        return (syn * 257).astype(np.uint16)
    if name == "uniform 16-bit noise":
        return np.random.default_rng(106 + seed).integers(0, 65536, (h, w)).astype(np.uint16)
    if name == "SYN-1 in the low byte":
        return syn.astype(np.uint16)
    if name == "uniform low byte under a constant even high byte":
        return (0x4000 + np.random.default_rng(107 + seed).integers(0, 256, (h, w))).astype(np.uint16)
    raise KeyError(name)


# The mode bit 0 each class must plan: fold where the image is a smooth signal sampled finer than a byte, plain where the
# low byte repeats the high byte, and plain -- a tie -- where the high byte never is odd.
# "uniform 16-bit noise" is NOT among them: on it the two encodes differ by 11 bytes of 131653 at -e1 and the two costs by
# 0.03 %, the cost walk and the oracle disagree (plain by cost, fold by 11 bytes), and either answer is a coin toss.  The
# constant-even-high-byte class stands in its place: noise again, and a tie that must plan as plain.
CLASSES = {"smooth 12-bit + N(0, 2)": 1, "smooth 12-bit + N(0, 8)": 1, "smooth 12-bit + N(0, 40)": 1, "SYN-1 x 16 + N(0, 4)": 1,
           "smooth x 16 + N(0, 30)": 1, "SYN-1 x 257": 0, "SYN-1 in the low byte": 0, "uniform low byte under a constant even high byte": 0}
TIES = ("SYN-1 in the low byte", "uniform low byte under a constant even high byte")
UNPLANNED = ("uniform 16-bit noise",)                           # a class of the byte comparison only (tools/deep_ab.py)
