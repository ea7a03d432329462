"""Sources for the collection's tests (tests/test_collect_host.py on the CPU, tests/test_encode_from_device.py on the GPU):
raw byte buffers in which an image's elements lie at a chosen residue, pitch and step, with NaN (0xFF bytes) wherever no
element lies, and the elements themselves as bit patterns for the numpy expression of the collected plane."""
import numpy as np

ELEM = (1, 2, 2, 4)
BITS = (np.uint8, np.uint16, np.uint16, np.uint32)
NORMS = ((1.0, 0.0), (255.0, 0.0), (127.5, 127.5))
WIDTHS = (1, 15, 16, 17, 33)
HEIGHTS = (1, 2, 3)
STEPS = (1, 3, 4)
GAP = 0xFF                                                     # NaN in float16, bfloat16 and float32; 255 as a pixel


def f32_bits(values):
    return np.ascontiguousarray(values, np.float32).view(np.uint32)


def element_bits(rng, fmt, shape):
    """Random elements of a format as bit patterns: pixels; or floats around [0, 1], around [0, 255] with halves, far
    outside, and every kind of special."""
    n = int(np.prod(shape))
    if fmt == 0:
        return rng.integers(0, 256, n, dtype=np.uint8).reshape(shape)
    f = np.empty(n, np.float32)
    kind = rng.integers(0, 8, n)
    f[:] = rng.random(n, np.float32)
    f = np.where(kind == 1, rng.integers(0, 512, n).astype(np.float32) * 0.5, f)
    f = np.where(kind == 2, rng.integers(-1000, 1000, n).astype(np.float32), f)
    f = np.where(kind == 3, rng.random(n, np.float32) * 2 - 0.5, f).astype(np.float32)
    bits = f32_bits(f).copy()
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x00000001, 0x807FFFFF], np.uint32)
    bits = np.where(kind == 4, special[rng.integers(0, 8, n)], bits)
    if fmt == 3:
        return bits.reshape(shape)
    if fmt == 2:
        return (bits >> 16).astype(np.uint16).reshape(shape)
    with np.errstate(over="ignore", invalid="ignore"):
        h = bits.view(np.float32).astype(np.float16).view(np.uint16)
    return np.where(kind == 5, rng.integers(0, 65536, n).astype(np.uint16), h).reshape(shape)


def as_values(bits, fmt):
    """The bit patterns as what collect_numpy takes: the format's floats (bfloat16: the patterns themselves)."""
    bits = np.ascontiguousarray(bits)
    return bits.view(np.float16) if fmt == 1 else (bits.view(np.float32) if fmt == 3 else bits)


def lay_out(bits, fmt, pitch, step, residue):
    """The raw bytes of a source: ``residue`` bytes of gap, then the elements of ``bits`` [rows, cols] ``pitch`` / ``step``
    bytes apart, gap bytes between them, and not a byte behind the last element."""
    rows, cols = bits.shape
    e = ELEM[fmt]
    extent = (rows - 1) * pitch + (cols - 1) * step + e
    raw = np.full(residue + extent, GAP, np.uint8)
    at = residue + np.arange(rows)[:, None] * pitch + np.arange(cols)[None, :] * step
    wide = bits.astype(np.uint32)
    for b in range(e):
        raw[at + b] = ((wide >> (8 * b)) & 0xFF).astype(np.uint8)
    return raw


def layouts(h, w, fmt, k):
    """(pitch, step) in bytes of the grid's four layouts: the three steps with a pitch that has slack, and transposed."""
    e = ELEM[fmt]
    out = [(((w - 1) * s + 1 + (k + i) % 4) * e, s * e) for i, s in enumerate(STEPS)]
    out.append((e, (h + k % 3) * e))                           # transposed: a row's pixels lie a column apart
    return out


def grid(fmt, seed=23):
    """The CPU grid of one format: every width, height, element-aligned residue modulo 16 and layout, as dicts with
    ``raw``, ``bits``, ``rows``, ``cols``, ``fmt``, ``pitch``, ``step``, ``residue``, ``scale``, ``bias``."""
    rng = np.random.default_rng(seed + fmt)
    e = ELEM[fmt]
    k = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            for residue in range(0, 16, e):
                for layout, (pitch, step) in enumerate(layouts(h, w, fmt, k)):
                    bits = element_bits(rng, fmt, (h, w))
                    scale, bias = NORMS[0] if fmt == 0 else NORMS[k % 3]
                    yield dict(raw=lay_out(bits, fmt, pitch, step, residue), bits=bits, rows=h, cols=w, fmt=fmt, pitch=pitch, step=step,
                               residue=residue, scale=scale, bias=bias, layout=layout)
                    k += 1


def all_patterns(fmt):
    """Every bit pattern of float16 (fmt 1) or bfloat16 (fmt 2) as one 256 x 256 image."""
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).reshape(256, 256)
