"""CPU suite: the delivery's unit walk (csrc/deliver.h, nblic_amd_debug_deliver_host) against numpy.  The kernel k_deliver
walks the same units with the same arithmetic, so what is checked here -- which bytes a window touches at every residue of
the destination, the two roundings of px * scale + bias, the conversions to float16 and bfloat16 -- is checked for both."""
import numpy as np
import pytest

WIDTHS = (1, 15, 16, 17, 131, 149, 150)
ROWS = 5
NORMS = ((1.0, 0.0), (1.0 / 255.0, -0.5), (0.0078125, -1.0))
ELEM = (1, 2, 2, 4)
PATTERN = 0x5A

_planes = {}


def plane_of(w, rows=ROWS):
    if (w, rows) not in _planes:
        p = np.random.default_rng(1000 + w).integers(0, 256, (rows, w), dtype=np.uint8)
        p.reshape(-1)[:2] = (0, 255)[: min(2, p.size)]
        p.setflags(write=False)
        _planes[(w, rows)] = p
    return _planes[(w, rows)]


def values(px, fmt, scale, bias):
    """The window's elements as the format's bytes, [rows, cols * elem]: numpy's float32 arithmetic, two roundings."""
    if fmt == 0:
        return np.ascontiguousarray(px)
    v = px.astype(np.float32) * np.float32(scale) + np.float32(bias)
    if fmt == 1:
        v = v.astype(np.float16)
    elif fmt == 2:                                             # round to nearest even on the float32 bits, in integers
        u = np.ascontiguousarray(v).view(np.uint32).astype(np.uint64)
        v = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.ascontiguousarray(v).view(np.uint8).reshape(px.shape[0], -1)


def expected(plane, window, fmt, scale, bias, pitch, offset, out_bytes, zero=False):
    r0, r1, c0, c1 = window
    out = np.full(out_bytes, PATTERN, np.uint8)
    rows = values(plane[r0:r1, c0:c1], fmt, scale, bias)
    if zero:
        rows = np.zeros_like(rows)
    for r in range(r1 - r0):
        out[offset + r * pitch: offset + r * pitch + rows.shape[1]] = rows[r]
    return out


def windows_of(w):
    wins = {(0, 1, 0, 1), (ROWS - 1, ROWS, w - 1, w), (0, ROWS, 0, w), (2, 3, 0, w), (0, ROWS, w // 2, w // 2 + 1), (ROWS - 1, ROWS, 0, w)}
    for c0 in range(17):
        for cols in (1, 15, 16, 17, 33):
            if c0 + cols <= w:
                wins.add((1, 4, c0, c0 + cols))
    return sorted(wins)


def layouts(fmt):
    """(slack of the pitch, offset of the destination) in bytes: every residue of 16 the format allows."""
    e = ELEM[fmt]
    slacks = (0, 1, 3) if fmt == 0 else (0, e)
    return [(s, o) for s in slacks for o in range(0, 16, e)]


@pytest.mark.parametrize("fmt", range(4))
@pytest.mark.parametrize("w", WIDTHS)
def test_windows_match_numpy(pkg, w, fmt):
    plane = plane_of(w)
    e = ELEM[fmt]
    for window in windows_of(w):
        cols, rows = window[3] - window[2], window[1] - window[0]
        for scale, bias in (NORMS[:1] if fmt == 0 else NORMS):
            for slack, offset in layouts(fmt):
                pitch = cols * e + slack
                out_bytes = offset + (rows - 1) * pitch + cols * e + 19
                info = {}
                got = pkg.deliver_host(plane, window, fmt, scale, bias, pitch=pitch, offset=offset, out_bytes=out_bytes, info=info)
                want = expected(plane, window, fmt, scale, bias, pitch, offset, out_bytes)
                assert np.array_equal(got, want), (w, fmt, window, scale, bias, slack, offset)
                assert (info["units"], info["chunks"]) == pkg.deliver_units(rows, cols, fmt) == (rows * ((cols + 16 // e - 1 + 15) // 16), 1)


@pytest.mark.parametrize("fmt", range(4))
def test_zero_flag_and_gate(pkg, fmt):
    plane = plane_of(149)
    window, e = (1, 4, 3, 36), ELEM[fmt]
    scale, bias = (1.0, 0.0) if fmt == 0 else (1.0 / 255.0, -0.5)
    pitch, offset = 33 * e + e, 3 * e
    out_bytes = offset + 2 * pitch + 33 * e + 7
    full = expected(plane, window, fmt, scale, bias, pitch, offset, out_bytes)
    zeros = expected(plane, window, fmt, scale, bias, pitch, offset, out_bytes, zero=True)
    assert not np.array_equal(full, zeros)
    call = lambda **kw: pkg.deliver_host(plane, window, fmt, scale, bias, pitch=pitch, offset=offset, out_bytes=out_bytes, **kw)
    assert np.array_equal(call(zero=True), zeros)                 # zero bytes (+0.0), not the bias, and nothing outside the rows
    assert np.array_equal(call(), full) and np.array_equal(call(gate_status=1), full)
    for status in (0, 2, 3, -2, 7):                            # running, starved, ...: anything but done
        assert np.array_equal(call(gate_status=status), zeros), status


def test_float16_roundings_at_the_edges_of_the_format(pkg):
    """Subnormal halves, ties, the smallest normal, overflow to infinity, negative zero: the integer conversion of the host
    walk against numpy's."""
    plane = np.arange(256, dtype=np.uint8).reshape(1, 256)
    norms = [(2.0 ** -24, 0.0), (2.0 ** -25, 0.0), (2.0 ** -26, 0.0), (1e-7, 0.0), (3e-8, 0.0), (2.0 ** -14 / 255, 0.0), (6.1e-5 / 100, 0.0), (257.0, 0.0),
             (256.94, 0.0), (300.0, -76000.0), (1.0, -65519.99), (-1e-7, 0.0), (-0.0, -0.0), (1.0009765625, 0.00048828125), (2.0 ** -24 * 1.5, 0.0),
             (3.0e38, 0.0), (0.333251953125, 2.0 ** -12), (1e-45, 0.0)]
    for scale, bias in norms:
        for fmt in (1, 2, 3):
            got = pkg.deliver_host(plane, (0, 1, 0, 256), fmt, scale, bias)
            with np.errstate(over="ignore"):
                want = values(plane, fmt, scale, bias).reshape(-1)
            assert np.array_equal(got, want), (scale, bias, fmt)


def test_unit_and_chunk_counts(pkg):
    plane = plane_of(150, 300)
    for fmt, per_row in ((0, 11), (1, 10), (2, 10), (3, 10)):     # (150 + 15 + 15) // 16, (150 + 7 + 15) // 16, (150 + 3 + 15) // 16
        info = {}
        pkg.deliver_host(plane, (0, 300, 0, 150), fmt, info=info)
        assert info == {"units": 300 * per_row, "chunks": (300 * per_row + 1023) // 1024}
        assert pkg.deliver_units(300, 150, fmt) == (info["units"], info["chunks"]) and info["chunks"] >= 3
    for cols, fmt, per_row in ((1, 0, 1), (2, 0, 2), (16, 0, 2), (17, 0, 2), (18, 0, 3), (1, 3, 1), (13, 3, 1), (14, 3, 2), (16, 1, 2), (9, 1, 1), (10, 2, 2)):
        info = {}
        pkg.deliver_host(plane, (7, 9, 3, 3 + cols), fmt, info=info)
        assert info["units"] == 2 * per_row, (cols, fmt)


def test_refusals(pkg):
    plane = plane_of(149)
    ok = dict(window=(1, 4, 3, 36), fmt=1, scale=0.5, bias=1.0, pitch=66, offset=2, out_bytes=2 + 2 * 66 + 66)
    pkg.deliver_host(plane, **ok)
    bad = [dict(fmt=4), dict(fmt=-1), dict(scale=float("nan")), dict(bias=float("inf")), dict(scale=float("-inf")), dict(fmt=0, scale=2.0, bias=0.0, pitch=33),
           dict(fmt=0, scale=1.0, bias=0.5, pitch=33), dict(window=(1, 1, 3, 36)), dict(window=(4, 1, 3, 36)), dict(window=(-1, 4, 3, 36)),
           dict(window=(1, ROWS + 1, 3, 36)), dict(window=(1, 4, 36, 36)), dict(window=(1, 4, -1, 32)), dict(window=(1, 4, 117, 150)), dict(pitch=64),
           dict(pitch=67), dict(offset=3, out_bytes=1000), dict(out_bytes=ok["out_bytes"] - 1), dict(offset=10 ** 6)]
    for change in bad:
        with pytest.raises(ValueError):
            pkg.deliver_host(plane, **{**ok, **change})
    with pytest.raises(ValueError):
        pkg.deliver_format("int32")
    assert [pkg.deliver_format(n) for n in ("uint8", "torch.float16", np.dtype("float32"), "torch.bfloat16")] == [0, 1, 3, 2]
