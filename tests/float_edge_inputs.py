"""The pixel conversions' arithmetic at its edges (tests/test_float_edges_host.py on the CPU, tests/test_float_edges.py on the
GPU): an EXACT reference for the contract of collect_value, deliver_value and deep_value, and the inputs on which a
conversion that breaks the contract gives another answer.  Everything here is pure CPU.

THE CONTRACT.  ``RN32(RN32(x * scale) + bias)``: two operations, each rounded to float32 to nearest even, subnormals kept,
never fused.  Then, for a source, the pixel rule (``!(v > 0)`` -> 0, ``v >= 255`` -> 255, else nearest, ties to even); for a
destination, the rounding to nearest even into float16 / bfloat16 (float32: the bits).

THE REFERENCE works on bit patterns with integers (numpy int64: a product of two 24-bit significands has 48 bits): no
float32 arithmetic of the hardware takes part in the operation under test.  It is written without a look at collect.h,
deliver.h, deep.h, ``collect_numpy`` or ``deep_inputs.value_bits``; the CPU suite compares it with numpy's float32 multiply
and add, with ``astype(np.float16)`` and, element by element in Python integers of any size, with ``scalar_bits``.

THE FUSED FORM ``RN32(x * scale + bias)``, one rounding, exists only to find WITNESSES: inputs on which it differs from the
contract in the final output (the pixel, the destination's bits).  Nothing is ever expected to equal it.  Witnesses have to
be constructed -- random pairs give none, the last rounding hides a last-place difference unless the value sits on a tie:
a scale whose product is inexact (float32(1/3): x = 3 j gives RN32(x * scale) = j exactly, the exact product is
j (1 + 2^-25)) and a bias that cancels into a finer binade, where the unfused sum lies exactly on a tie and the fused one a
little above it.

WHAT THE SEARCH FINDS FOR 8-BIT PIXELS.  With a bias of plain shape the sum's binade is coarser than the product's error
and no half format has a witness ((1/255, -0.5): 158 in float32, 0 in float16).  A bias that cancels AND carries a tie
offset does better: under float32(1/3) / 64 and -0.5 + 2^-12 the pixels 3 j, j = 64 .. 85, land on 2^-12 above a float16
in [0.5, 1) -- a tie -- and the fused sum a little higher.  The family searched is stated at ``DELIVER_FAMILY``; what it
finds is ``DELIVER_FOUND`` -- 21 witnesses in float16, 16 in bfloat16, 158 in float32 -- and the CPU suite runs the search
and asserts exactly those pairs and numbers.

ONE CORRECTION to what was asked of the float32 subnormal elements: under a scale of 3e38 (the largest there is, nearly)
a subnormal of 2^-149 becomes 4.2e-7, which is pixel 0 whether it was flushed or not.  Only subnormals of 2^-128 and above
reach 0.5.  ``F32_SUBNORMALS`` therefore holds the 23 one-bit ones and the two largest, as asked, AND a dense run of large
ones; the CPU suite asserts that every one whose exact product exceeds 0.5 gives a pixel that is not the flushed one, and
that there are at least 64 of them."""
import struct

import numpy as np

import collect_inputs

I64 = np.int64

# ---- the formats: (significand bits with the hidden one, exponent of the smallest subnormal, exponent field's maximum, bits) ----
F32 = (24, -149, 255, 32)
F16 = (11, -24, 31, 16)
BF16 = (8, -133, 255, 16)
FORMAT = {1: F16, 2: BF16, 3: F32}                               # by the collect / deliver format number
NAMES = {1: "float16", 2: "bfloat16", 3: "float32"}
ELEM = {1: 2, 2: 2, 3: 4}


def f32(v):
    """The bits of the float32 nearest to a Python float (a conversion, not an operation under test)."""
    return struct.unpack("<I", struct.pack("<f", v))[0]


def f32_value(v):
    """The Python float that is exactly the float32 nearest to ``v``."""
    return struct.unpack("<f", struct.pack("<f", v))[0]


THIRD = f32_value(1.0 / 3.0)                                     # 0x3EAAAAAB: 1/3 (1 + 2^-25)


# ---- integer soft-float, vectorised -----------------------------------------------------------------------------------------
def _bitlen(m):
    """bit_length of every element of a non-negative int64 array."""
    t = m.copy()
    n = np.zeros(m.shape, I64)
    for s in (32, 16, 8, 4, 2, 1):
        big = t >= (I64(1) << s)
        n += np.where(big, s, 0)
        t = np.where(big, t >> s, t)
    return n + (t > 0)


def _decode(bits, fmt=F32):
    """(sign, m, e, nan, inf) of bit patterns of a format: a finite value is (-1)^sign * m * 2^e."""
    p, qmin, top, width = fmt
    b = np.asarray(bits).astype(I64)
    sign = (b >> (width - 1)) & 1
    field = (b >> (p - 1)) & top
    frac = b & ((1 << (p - 1)) - 1)
    m = np.where(field == 0, frac, frac | (1 << (p - 1)))
    e = np.where(field == 0, qmin, field - 1 + qmin)
    special = field == top
    m = np.where(special, 0, m)
    return sign, m, e, special & (frac != 0), special & (frac == 0)


def _of_int(v):
    """Integers as decoded values: exact."""
    v = np.asarray(v).astype(I64)
    no = np.zeros(v.shape, bool)
    return (v < 0).astype(I64), np.abs(v), np.zeros(v.shape, I64), no, no


def _pack(sign, m, e, fmt=F32):
    """The bits of (-1)^sign * m * 2^e (m < 2^62, exact) rounded to nearest even into a format: subnormals as they are, an
    overflow to infinity."""
    p, qmin, top, width = fmt
    q = np.where(m == 0, qmin, np.maximum(_bitlen(m) - p + e, qmin))      # the exponent of the result's unit in the last place
    down = np.clip(q - e, 0, 63)
    up = np.clip(e - q, 0, 63)
    r = (m >> down) << up
    rem = m - ((m >> down) << down)
    half = np.where(down > 0, I64(1) << np.maximum(down - 1, 0), 0)
    r = r + ((down > 0) & ((rem > half) | ((rem == half) & ((r & 1) == 1))))
    body = ((q - qmin) << (p - 1)) + r                          # (a carry into 2^p moves into the exponent field by itself)
    body = np.minimum(body, I64(top) << (p - 1))
    return ((sign << (width - 1)) | body).astype(np.uint32)


def _nan_inf(sign, nan, inf, bits, fmt=F32):
    p, _, top, width = fmt
    bits = np.where(inf, (sign << (width - 1)) | (I64(top) << (p - 1)), bits.astype(I64))
    return np.where(nan, (I64(top) << (p - 1)) | (1 << (p - 2)), bits).astype(np.uint32)


def _mul(a, b):
    """RN32(a * b) of two decoded values: bits."""
    sa, ma, ea, na, ia = a
    sb, mb, eb, nb, ib = b
    sign = sa ^ sb
    nan = na | nb | (ia & (mb == 0) & ~ib) | (ib & (ma == 0) & ~ia)
    return _nan_inf(sign, nan, (ia | ib) & ~nan, _pack(sign, ma * mb, ea + eb))


def _add(a, b):
    """RN32(a + b) of two decoded float32 values (m < 2^24): bits."""
    sa, ma, ea, na, ia = a
    sb, mb, eb, nb, ib = b
    nan = na | nb | (ia & ib & (sa != sb))
    inf = (ia | ib) & ~nan
    swap = ea < eb
    s1, m1, e1 = np.where(swap, sb, sa), np.where(swap, mb, ma), np.where(swap, eb, ea)
    s2, m2, e2 = np.where(swap, sa, sb), np.where(swap, ma, mb), np.where(swap, ea, eb)
    e2 = np.where(m2 == 0, e1, e2)                              # (a zero has the smallest exponent there is: it is never the first)
    # far below the first one's last place, the second decides nothing but the side: 0 < it < 2^(e1 - 6) stands for it
    far = e1 - e2 > 30
    m2 = np.where(far, 1, m2)
    e2 = np.where(far, e1 - 30, e2)
    total = np.where(s1 == 1, -1, 1) * (m1 << (e1 - e2)) + np.where(s2 == 1, -1, 1) * m2
    sign = np.where(total == 0, sa & sb, (total < 0).astype(I64))      # (an exact zero: +0 unless both are negative)
    return _nan_inf(np.where(ia, sa, sb), nan, inf, _pack(sign, np.abs(total), e2))


def contract_f32(x, scale, bias):
    """RN32(RN32(x * scale) + bias): ``x`` decoded, ``scale`` and ``bias`` Python floats (their nearest float32); bits."""
    s, b = _decode(np.uint32(f32(scale))), _decode(np.uint32(f32(bias)))
    return _add(_decode(_mul(x, s)), b)


def widen(bits, fmt):
    """float16 / bfloat16 / float32 bit patterns -> the decoded values (exact)."""
    return _decode(bits, FORMAT[fmt])


def widen_bits(bits, fmt):
    """The float32 bits of float16 / bfloat16 elements: exact, NaN as a quiet NaN."""
    s, m, e, nan, inf = widen(bits, fmt)
    return _nan_inf(s, nan, inf, _pack(s, m, e))


def narrow_bits(bits32, fmt):
    """float32 bits -> the destination's bits, to nearest even; bfloat16 NaN: the upper half with bit 6 set."""
    bits32 = np.asarray(bits32, np.uint32)
    if fmt == 3:
        return bits32.copy()
    s, m, e, nan, inf = _decode(bits32)
    out = _nan_inf(s, np.zeros(nan.shape, bool), inf, _pack(s, m, e, FORMAT[fmt]), FORMAT[fmt])
    quiet = (s << 15) | 0x7E00 if fmt == 1 else (bits32.astype(I64) >> 16) | 0x40
    return np.where(nan, quiet, out).astype(np.uint32)


def pixel_of(bits32):
    """The pixel rule on float32 bits: uint8."""
    s, m, e, nan, inf = _decode(bits32)
    down = np.clip(-e, 0, 63)
    whole = np.where(e >= 0, m << np.clip(e, 0, 8), m >> down)          # (m * 2^e >= 2^23 when e >= 0: clamped below anyway)
    rem = np.where(e >= 0, 0, m - ((m >> down) << down))
    half = np.where(down > 0, I64(1) << np.maximum(down - 1, 0), 0)
    near = whole + ((e < 0) & ((rem > half) | ((rem == half) & (rem > 0) & ((whole & 1) == 1))))
    px = np.where(inf | (whole >= 255), 255, near)
    px = np.where(nan | (s == 1) | ((m == 0) & ~inf), 0, px)
    return px.astype(np.uint8)


# ---- the same in Python integers of any size, one element at a time: the fused form, and a second opinion --------------------
def _rn_scalar(num, e, fmt=F32):
    """The bits of num * 2^e (num a signed Python integer, not 0) rounded to nearest even into a format."""
    p, qmin, top, width = fmt
    sign, mag = (1 if num < 0 else 0), abs(num)
    q = max(mag.bit_length() - p + e, qmin)
    if q <= e:
        r = mag << (e - q)
    else:
        k = q - e
        r, rem = mag >> k, mag & ((1 << k) - 1)
        if rem > (1 << (k - 1)) or (rem == (1 << (k - 1)) and r & 1):
            r += 1
    return (sign << (width - 1)) | min(((q - qmin) << (p - 1)) + r, top << (p - 1))


def _dec_scalar(bits):
    field, frac = (bits >> 23) & 255, bits & 0x7FFFFF
    return (-1 if bits >> 31 else 1) * (frac if field == 0 else frac | 0x800000), (-149 if field == 0 else field - 150)


def scalar_bits(sx, mx, ex, scale, bias, fused):
    """One finite element (-1)^sx * mx * 2^ex under finite scale and bias, in Python integers: the contract's float32 bits, or
    (``fused``) RN32(x * scale + bias) with ONE rounding.  An overflowing product is infinite in the contract only."""
    ms, es = _dec_scalar(f32(scale))
    mb, eb = _dec_scalar(f32(bias))
    num, e = (-mx if sx else mx) * ms, ex + es
    psign = sx ^ (1 if ms < 0 or (ms == 0 and f32(scale) >> 31) else 0)
    if not fused:
        pbits = _rn_scalar(num, e) if num else psign << 31
        if pbits & 0x7FFFFFFF == 0x7F800000:
            return pbits
        num, e = _dec_scalar(pbits)
        if num == 0:
            psign = pbits >> 31
    low = min(e, eb)
    total = (num << (e - low)) + (mb << (eb - low))
    if total == 0:
        return (psign & (f32(bias) >> 31)) << 31 if num == 0 and mb == 0 else 0
    return _rn_scalar(total, low)


def fused_f32(x, scale, bias):
    """RN32(x * scale + bias), one rounding, of decoded values: the contract's bits wherever the product is exact or the
    bias is zero (nothing to fuse), Python integers elsewhere."""
    two = contract_f32(x, scale, bias)
    if bias == 0.0:
        return two
    sx, mx, ex, nan, inf = (np.asarray(v).reshape(-1) for v in x)
    ss, ms, es, _, _ = _decode(np.uint32(f32(scale)))
    prod = mx * ms
    width = _bitlen(prod) - _bitlen(prod & -prod) + 1           # significant bits of the product
    field = (_mul(x, _decode(np.uint32(f32(scale)))).astype(I64).reshape(-1) >> 23) & 255
    inexact = ~nan & ~inf & (prod != 0) & ((width > 24) | (field == 0) | (field == 255))
    out = two.copy().reshape(-1)
    for i in np.flatnonzero(inexact):
        out[i] = scalar_bits(int(sx[i]), int(mx[i]), int(ex[i]), scale, bias, True)
    return out.reshape(two.shape)


# ---- the three conversions ------------------------------------------------------------------------------------------------------
def collect_ref(bits, fmt, scale, bias, fused=False):
    """The pixels (uint8) of source elements given as bit patterns of format 1, 2 or 3."""
    return pixel_of((fused_f32 if fused else contract_f32)(widen(bits, fmt), scale, bias))


def deliver_ref(px, fmt, scale, bias, fused=False):
    """The destination's bits (uint32) of pixels, or of any integers (a deep image's values)."""
    return narrow_bits((fused_f32 if fused else contract_f32)(_of_int(px), scale, bias), fmt)


def deep_ref(u, signed, fmt, scale, bias, fused=False):
    """The destination's bits of the 16-bit values ``u`` (as unsigned numbers) of a deep image; ``fmt`` 1, 2, 3 as above."""
    return deliver_ref(np.asarray(u).astype(I64) - (32768 if signed else 0), fmt, scale, bias, fused)


def witnesses(want, fused):
    return int((np.asarray(want) != np.asarray(fused)).sum())


# ---- collect: the witness sets ------------------------------------------------------------------------------------------------
COLLECT_WITNESS_PAIR = {1: (THIRD, -299.5), 2: (THIRD, -41.5), 3: (f32_value(1234.567), -617.25)}
COLLECT_WITNESS_MIN = {1: 100, 2: 50, 3: 64}


def f32_neighbourhoods(scale, bias, radius=64, clamps=False):
    """float32 bit patterns within ``radius`` units in the last place of (k + 0.5 - bias) / scale, k = 0 .. 254 -- the ties of
    the pixel rule -- or (``clamps``) of the elements that give v = 0 and v = 255."""
    at = np.array([0.0, 255.0]) if clamps else np.arange(255) + 0.5
    with np.errstate(over="ignore"):
        centre = ((at - bias) / scale).astype(np.float32)
    centre = centre[np.isfinite(centre)]
    sign = centre.view(np.uint32) & np.uint32(0x80000000)
    mag = (centre.view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(I64)[:, None] + np.arange(-radius, radius + 1)[None, :]
    mag = np.clip(mag, 0, 0x7F7FFFFF)
    return (mag.astype(np.uint32) | sign[:, None]).reshape(-1)


def collect_witness_inputs(fmt):
    """The elements (bit patterns, 1-D) of the witness set of a format: see the table in the module's docstring."""
    scale, bias = COLLECT_WITNESS_PAIR[fmt]
    if fmt == 3:
        return f32_neighbourhoods(scale, bias)
    bits = np.arange(0x7C00 if fmt == 1 else 0x7F80, dtype=np.uint32)      # the positive finite patterns
    s, m, e, _, _ = _decode(contract_f32(widen(bits, fmt), scale, bias))
    v2 = np.where(s == 1, -1, 1) * np.where(e >= -1, m << np.clip(e + 1, 0, 8), m >> np.clip(-e - 1, 0, 63))      # about 2 v
    return bits[(v2 > -3) & (v2 < 517) & (e < 0)]              # -1.5 < v < 258.5


NORMALISE = (f32_value(255.0 / 0.229), f32_value(-0.485 / 0.229 * 255.0))          # ImageNet's first channel onto 0 .. 255: full-width significands
COLLECT_PAIRS = (COLLECT_WITNESS_PAIR[1], COLLECT_WITNESS_PAIR[2], (-255.0, 255.0), (0.0, 0.0), (0.0, 7.5), (3e38, 0.0), (-3e38, 255.0), NORMALISE)
F32_SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x00000001, 0x807FFFFF,      # element_bits' own
                         0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x80800000, 0x3F000000, 0x3F800000, 0x437F0000, 0x437E8000], np.uint32)
F32_SUBNORMALS = np.concatenate([np.uint32(1) << np.arange(23, dtype=np.uint32), np.array([0x007FFFFF, 0x807FFFFF], np.uint32),
                                 (0x00200000 + 0x0001E0F1 * np.arange(48)).astype(np.uint32),
                                 (0x80200000 + 0x0001E0F1 * np.arange(48)).astype(np.uint32)])


def f32_collect_inputs(scale, bias):
    """The float32 elements for one pair: the tie and clamp neighbourhoods (none under a scale of 0), the specials, the
    subnormals."""
    parts = [F32_SPECIALS, F32_SUBNORMALS]
    if scale != 0.0:
        parts += [f32_neighbourhoods(scale, bias), f32_neighbourhoods(scale, bias, clamps=True)]
    return np.concatenate(parts)


def as_image(bits, cols, fill):
    """1-D elements as a 2-D image of ``cols`` columns, the last row filled up with ``fill``."""
    n = -(-bits.size // cols) * cols
    return np.concatenate([bits, np.full(n - bits.size, fill, bits.dtype)]).reshape(-1, cols)


def collect_domains():
    """Every collect domain as a dict with ``name``, ``fmt``, ``scale``, ``bias``, ``bits`` (2-D: uint16 for the half formats,
    uint32 for float32).  The shapes are odd on purpose: rows end inside units."""
    out = []
    for fmt in (1, 2, 3):
        scale, bias = COLLECT_WITNESS_PAIR[fmt]
        w = collect_witness_inputs(fmt)
        out.append(dict(name="witness set", fmt=fmt, scale=scale, bias=bias, bits=as_image(w, 37, w[0]).astype(collect_inputs.BITS[fmt])))
    for fmt in (1, 2):
        for scale, bias in COLLECT_PAIRS:
            out.append(dict(name="all patterns", fmt=fmt, scale=scale, bias=bias, bits=collect_inputs.all_patterns(fmt)))
    for scale, bias in COLLECT_PAIRS:
        b = f32_collect_inputs(scale, bias)
        out.append(dict(name="float32 edges", fmt=3, scale=scale, bias=bias, bits=as_image(b, 131, b[0])))
    return out


_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def collect_expected():
    """[(domain, pixels by the exact reference)], computed once and left unchanged."""
    return memo("collect", lambda: [(d, collect_ref(d["bits"], d["fmt"], d["scale"], d["bias"])) for d in collect_domains()])


def collect_task(d, layout, k=0):
    """A domain as a task of ``Context.debug_collect``: ``contiguous`` (aligned words), or ``strided`` (step 3 elements, an
    odd residue: element by element)."""
    e = ELEM[d["fmt"]]
    rows, cols = d["bits"].shape
    if layout == "contiguous":
        pitch, step, residue = cols * e, e, 0
    else:
        pitch, step, residue = (cols * 3 + 1 + k % 3) * e, 3 * e, e * (1 + 2 * (k % 2))
    raw = collect_inputs.lay_out(d["bits"], d["fmt"], pitch, step, residue)
    return dict(raw=raw[residue:], rows=rows, cols=cols, fmt=d["fmt"], pitch=pitch, step=step, scale=d["scale"], bias=d["bias"],
                base_offset=residue + 16 * (k % 15))


def collect_ref_task():
    """One task with a REFERENCE: the float16 witness set against itself turned round, so both channels hold witnesses.
    (task of ``Context.debug_collect_ref``, the two sources' bits, the expected plane)."""
    def make():
        d = collect_domains()[0]
        own, ref = d["bits"], np.ascontiguousarray(d["bits"][::-1, ::-1])
        t = collect_task(d, "contiguous")
        t.update(ref=ref, ref_base_offset=6)
        a, b = (collect_ref(x, 1, d["scale"], d["bias"]).astype(I64) for x in (own, ref))
        return t, own, ref, ((a - b + 128) % 256).astype(np.uint8)
    return memo("collect ref", make)


# ---- deliver --------------------------------------------------------------------------------------------------------------------
PATTERN = 0x5A                                                   # what every destination buffer holds before a walk or a launch
TAIL = 24                                                        # bytes of it behind every destination
# The family searched for 8-bit pixels: scale float32(1/3) * 2^a or float32(1/255) * 2^a, a = -6 or 0 (another power of two
# moves scale and bias alike and changes nothing short of the formats' ends), and a bias -2^c + t * 2^(c-12) with
# c = a - 3 .. a + 8 and t = 0, +-1, +-2, +-3: a cancellation, and an offset that puts the sums on ties.
DELIVER_FAMILY = [(f32_value(base * 2.0 ** a), -(2.0 ** c) + t * 2.0 ** (c - 12)) for base in (THIRD, f32_value(1 / 255)) for a in (-6, 0)
                  for c in range(a - 3, a + 9) for t in (0, 1, -1, 2, -2, 3, -3)]
PIXELS = np.arange(256, dtype=I64)


def deliver_search():
    """Per format the first pair of the family with the most witnesses among the 256 pixels: {fmt: (count, scale, bias)}."""
    best = {}
    for scale, bias in DELIVER_FAMILY:
        two, one = contract_f32(_of_int(PIXELS), scale, bias), fused_f32(_of_int(PIXELS), scale, bias)
        for fmt in (1, 2, 3):
            n = witnesses(narrow_bits(two, fmt), narrow_bits(one, fmt))
            if fmt not in best or n > best[fmt][0]:
                best[fmt] = (n, scale, bias)
    return best


# What deliver_search() finds, {fmt: (witnesses, scale, bias)}: the CPU suite runs the search and compares.
DELIVER_FOUND = {1: (21, f32_value(THIRD / 64), -0.5 + 2.0 ** -12), 2: (16, f32_value(THIRD / 64), -1.0 + 2.0 ** -11),
                 3: (158, f32_value(f32_value(1 / 255) / 64), -(2.0 ** -7))}
DELIVER_F32_PAIR = (f32_value(1 / 255), -0.5)                   # 158 float32 witnesses by itself
DELIVER_TIE_PAIRS = ((1.0, 2048.0), (1.0, 256.0))               # odd pixels on float16 ties; on bfloat16 ties
DELIVER_ZERO_PAIRS = ((-1.0, 0.0), (-1.0, -0.0))                # pixel 0: -0 + 0 = +0, -0 + -0 = -0
DELIVER_PAIRS = tuple(DELIVER_FOUND[f][1:] for f in (1, 2, 3)) + (DELIVER_F32_PAIR,) + DELIVER_TIE_PAIRS + DELIVER_ZERO_PAIRS
PIXEL_PLANE = (np.arange(7 * 41) % 256).astype(np.uint8).reshape(7, 41)      # all 256 pixels; rows that are no multiple of a unit


def scatter(bits, elem, offset, pitch, step, size):
    """A buffer of ``size`` bytes of the pattern with the elements ``bits`` (2-D) laid ``pitch`` / ``step`` bytes apart from
    byte ``offset`` on."""
    out = np.full(size, PATTERN, np.uint8)
    rows, cols = np.mgrid[0:bits.shape[0], 0:bits.shape[1]]
    at = offset + rows * pitch + cols * step
    for b in range(elem):
        out[at + b] = (np.asarray(bits).astype(np.uint64) >> np.uint64(8 * b)) & np.uint64(0xFF)
    return out


def _dest(k, rows, cols, elem, strided):
    """offset, pitch, step and size of destination k: a head in front of the first unit, pattern bytes behind the last."""
    step = 3 * elem if strided else elem
    pitch = cols * step + (2 * elem if k % 2 else 0)
    offset = 16 + elem * (1 + k % 3)
    return dict(offset=offset, pitch=pitch, step=step, out_bytes=offset + (rows - 1) * pitch + (cols - 1) * step + elem + TAIL)


def deliver_tasks():
    """[(task of ``Context.debug_deliver``, expected buffer)]: all 256 pixels into every float format under every pair of
    DELIVER_PAIRS, contiguous and -- every third -- strided."""
    def make():
        out, k = [], 0
        rows, cols = PIXEL_PLANE.shape
        for fmt in (1, 2, 3):
            for scale, bias in DELIVER_PAIRS:
                d = _dest(k, rows, cols, ELEM[fmt], k % 3 == 2)
                want = deliver_ref(PIXEL_PLANE, fmt, scale, bias)
                out.append((dict(d, plane=PIXEL_PLANE, window=(0, rows, 0, cols), fmt=fmt, scale=scale, bias=bias, base_offset=k % 16),
                            scatter(want, ELEM[fmt], d["offset"], d["pitch"], d["step"], d["out_bytes"])))
                k += 1
        return out
    return memo("deliver", make)


def deliver_ref_tasks():
    """The same for a delivery with a REFERENCE plane (``Context.debug_deliver_ref``): the plane holds differences, the pixel
    is (plane + ref - 128) & 255, all 256 values again; one task per format under its witness pair."""
    def make():
        out = []
        rows, cols = PIXEL_PLANE.shape
        base = ((PIXEL_PLANE.astype(I64) * 29 + 7) % 256).astype(np.uint8)
        diff = ((PIXEL_PLANE.astype(I64) - base + 128) % 256).astype(np.uint8)
        for k, fmt in enumerate((1, 2, 3)):
            _, scale, bias = DELIVER_FOUND[fmt]
            d = _dest(k, rows, cols, ELEM[fmt], fmt == 2)
            want = deliver_ref(PIXEL_PLANE, fmt, scale, bias)
            out.append((dict(d, plane=diff, ref=base, window=(0, rows, 0, cols), fmt=fmt, scale=scale, bias=bias, base_offset=3 + k, ref_base_offset=9 - k),
                        scatter(want, ELEM[fmt], d["offset"], d["pitch"], d["step"], d["out_bytes"])))
        return out
    return memo("deliver ref", make)


# ---- deep deliver ---------------------------------------------------------------------------------------------------------------
DEEP_SHAPE = (241, 272)                                          # 65552 elements: every 16-bit value, the first sixteen twice
DEEP_U = (np.arange(DEEP_SHAPE[0] * DEEP_SHAPE[1]) % 65536).reshape(DEEP_SHAPE)
DEEP_PAIRS = {"identity": (1.0, 0.0),                            # float16: 65520 and above overflow; ties in both half formats
              "witness": (THIRD, -8192.0),                       # u = 3 j: j exactly, against j (1 + 2^-25) fused, on ties after the bias
              "tiny": (2.0 ** -30, 0.0),                         # float16 subnormals, and ties among them
              "negative": (-THIRD, 8192.0),                      # the witness pair turned round
              "huge": (3e38, 0.0)}                               # overflow in bfloat16 and float32
DEEP_FMT = {1: 2, 2: 3, 3: 4}                                    # the deep calls' own numbering of the destination formats


def on_tie(bits32, fmt):
    """Which float32 bit patterns lie exactly halfway between two neighbours of a half format (normal results only)."""
    b = np.asarray(bits32).astype(I64)
    mag = b & 0x7FFFFFFF
    if fmt == 2:
        return ((b & 0xFFFF) == 0x8000) & (mag < 0x7F7F0000)
    return ((b & 0x1FFF) == 0x1000) & (mag >= 0x38800000) & (mag < 0x477FE000)


def deep_f32(name, signed, fused=False):
    """The float32 bits of every value of DEEP_U under a pair, by the contract (or fused): computed once."""
    scale, bias = DEEP_PAIRS[name]
    return memo(("deep", name, signed, fused), lambda: (fused_f32 if fused else contract_f32)(_of_int(DEEP_U - (32768 if signed else 0)), scale, bias))


def deep_regimes():
    """{(regime, fmt): count} of what the deep domain reaches by the reference, signed and unsigned together."""
    def make():
        r = {}
        for fmt in (1, 2, 3):
            field_top, shift, mant = (31, 10, 0x3FF) if fmt == 1 else (255, 7 if fmt == 2 else 23, 0x7F if fmt == 2 else 0x7FFFFF)
            inf = sub = tie = neg = wit = 0
            for name in DEEP_PAIRS:
                for signed in (False, True):
                    two = deep_f32(name, signed).reshape(-1)[:65536]
                    out = narrow_bits(two, fmt).astype(I64)
                    field = (out >> shift) & field_top
                    inf += int(((field == field_top) & ((out & mant) == 0)).sum())
                    sub += int(((field == 0) & ((out & mant) != 0)).sum())
                    if fmt != 3:
                        tie += int(on_tie(two, fmt).sum())
                    if DEEP_PAIRS[name][0] < 0:
                        neg += 65536
                    if name == "witness":
                        wit += witnesses(out, narrow_bits(deep_f32(name, signed, True).reshape(-1)[:65536], fmt))
            r.update({("infinite", fmt): inf, ("subnormal", fmt): sub, ("tie", fmt): tie, ("negative scale", fmt): neg, ("witness", fmt): wit})
        return r
    return memo("deep regimes", make)


def deep_tasks():
    """[(task of ``Context.debug_deep_deliver``, expected buffer)]: every 16-bit value, unsigned and signed, into the three
    float formats under every pair; the low plane folded in every other task."""
    def make():
        out, k = [], 0
        rows, cols = DEEP_SHAPE
        hi, lo = (DEEP_U >> 8).astype(np.uint8), (DEEP_U & 255).astype(np.uint8)
        folded = np.where(hi & 1, 255 - lo, lo).astype(np.uint8)
        for fmt in (1, 2, 3):
            for name, (scale, bias) in DEEP_PAIRS.items():
                for signed in (False, True):
                    mode = (2 if signed else 0) | (k & 1)
                    d = _dest(k, rows, cols, ELEM[fmt], k % 5 == 4)
                    want = narrow_bits(deep_f32(name, signed), fmt)
                    out.append((dict(d, hi=hi, lo=folded if mode & 1 else lo, window=(0, rows, 0, cols), fmt=DEEP_FMT[fmt], mode=mode, scale=scale, bias=bias,
                                     base_offsets=(k % 16, (3 * k + 1) % 16), pair=name),
                                scatter(want, ELEM[fmt], d["offset"], d["pitch"], d["step"], d["out_bytes"])))
                    k += 1
        return out
    return memo("deep tasks", make)


# ---- stack deliver ----------------------------------------------------------------------------------------------------------------
def stack_tasks():
    """[(task of ``Context.debug_stack_deliver``, [expected buffer per slice], the restored slices)]: one run of a key and two
    deltas whose restored bytes are all 256 values in every slice, per float format, a witness pair per slice."""
    def make():
        out = []
        x0 = np.arange(256, dtype=I64).reshape(8, 32)
        slices = [x0, (x0 * 37 + 11) % 256, 255 - x0]
        planes = [slices[0].astype(np.uint8)] + [((slices[d] - slices[d - 1] + 128) % 256).astype(np.uint8) for d in (1, 2)]
        for k, fmt in enumerate((1, 2, 3)):
            pairs = [DELIVER_FOUND[fmt][1:], DELIVER_F32_PAIR, DELIVER_FOUND[1 + fmt % 3][1:]]
            e = ELEM[fmt]
            dests = [_dest(k + d, 8, 32, e, d == 2) for d in range(3)]
            task = dict(planes=planes, window=(0, 8, 0, 32), fmt=fmt, scales=[p[0] for p in pairs], biases=[p[1] for p in pairs],
                        steps=[d["step"] for d in dests], pitches=[d["pitch"] for d in dests], offsets=[d["offset"] for d in dests],
                        out_bytes=[d["out_bytes"] for d in dests], base_offsets=[(5 * d + k) % 16 for d in range(3)])
            want = [scatter(deliver_ref(x, fmt, *p), e, d["offset"], d["pitch"], d["step"], d["out_bytes"]) for x, p, d in zip(slices, pairs, dests)]
            out.append((task, want, slices))
        return out
    return memo("stack", make)


# ---- the cost kernels: float sources through the collection's loader -----------------------------------------------------------------
COST_SHAPE = (65, 130)                                           # more than one tile both ways
HALF_SPECIALS = np.array([0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0x0001, 0x83FF, 0x7BFF], np.uint32)


def cost_planes(fmt, count, seed):
    """``count`` images of COST_SHAPE whose elements are drawn from the format's witness set and the specials:
    [(bits, pixels by the exact reference)], under the format's witness pair."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([collect_witness_inputs(fmt), F32_SPECIALS if fmt == 3 else HALF_SPECIALS])
    scale, bias = COLLECT_WITNESS_PAIR[fmt]
    out = []
    for _ in range(count):
        bits = pool[rng.integers(0, pool.size, COST_SHAPE)].astype(collect_inputs.BITS[fmt])
        out.append((bits, collect_ref(bits, fmt, scale, bias)))
    return out


def cost_tasks():
    """[(task of ``Context.debug_color_cost`` / ``debug_stack_cost``, the reference-collected planes)] for ("color" | "stack",
    float16 | float32): the float16 frame and the float32 stack contiguous, the other two interleaved."""
    def make():
        out = {}
        rows, cols = COST_SHAPE
        for kind in ("color", "stack"):
            for fmt in (1, 3):
                e = ELEM[fmt]
                step = e if (kind == "color") == (fmt == 1) else 3 * e
                pitch = cols * step + 2 * e
                made = cost_planes(fmt, 3, 40 + fmt + (10 if kind == "stack" else 0))
                scale, bias = COLLECT_WITNESS_PAIR[fmt]
                task = dict(raws=[collect_inputs.lay_out(b, fmt, pitch, step, 0) for b, _ in made], rows=rows, cols=cols, fmt=fmt, pitches=[pitch] * 3,
                            steps=[step] * 3, scale=scale, bias=bias, base_offsets=[(2 * d + 1) * e for d in range(3)])
                out[(kind, fmt)] = (task, [p for _, p in made])
        return out
    return memo("cost", make)


def first_difference(got, want):
    """The flat index of the first element in which two arrays differ."""
    return int(np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))[0])


# ---- what a failure says ------------------------------------------------------------------------------------------------------------
def explain_plane(what, fmt, scale, bias, bits, got, want):
    """For a collected plane that differs: format, scale, bias and the first differing element with its input bits."""
    i = first_difference(got, want)
    return "%s: %s scale %r bias %r: %d of %d pixels differ, first element %d with bits 0x%X: got %d, the contract gives %d" % (
        what, NAMES[fmt], scale, bias, int((np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1)).sum()), np.asarray(want).size, i,
        int(np.asarray(bits).reshape(-1)[i]), int(np.asarray(got).reshape(-1)[i]), int(np.asarray(want).reshape(-1)[i]))


def explain_buffer(what, fmt, scale, bias, task, values, got, want):
    """For a destination buffer that differs: format, scale, bias, the first differing byte, and -- inside the window -- its
    element with the input value and both results' bits.  ``values``: the window's inputs (pixels, or a deep image's values)."""
    i = first_difference(got, want)
    e, cols = ELEM[fmt], np.asarray(values).shape[1]
    head = "%s: %s scale %r bias %r: byte %d of the buffer differs (got 0x%02X, want 0x%02X)" % (what, NAMES[fmt], scale, bias, i, int(got[i]), int(want[i]))
    rel = i - task["offset"]
    row, col = rel // task["pitch"], (rel % task["pitch"]) // task["step"] if rel >= 0 else -1
    if rel < 0 or row >= np.asarray(values).shape[0] or col >= cols or (rel % task["pitch"]) % task["step"] >= e:
        return head + ": a byte OUTSIDE every element"
    at = task["offset"] + row * task["pitch"] + col * task["step"]
    word = lambda buf: int.from_bytes(bytes(buf[at:at + e]), "little")
    return head + ": element (%d, %d), input %d: got bits 0x%X, the contract gives 0x%X" % (row, col, int(np.asarray(values)[row, col]), word(got), word(want))


