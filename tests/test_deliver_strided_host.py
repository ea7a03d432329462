"""CPU suite: the STRIDED delivery task (csrc/deliver.h: the elements of a destination row lie ``step`` bytes apart) through
the host walk, nblic_amd_debug_deliver_host_ex, against a numpy scatter.  The kernel's strided path visits the same
elements with the same arithmetic (tests/test_decode_to_layouts.py compares the two byte for byte), so which bytes a strided
window touches -- and which it leaves alone -- is checked here for both."""
import numpy as np
import pytest

ROWS, WIDTH = 5, 149
ELEM = (1, 2, 2, 4)
PATTERN = 0x5A
STEPS = (2, 3, 4, 7)                                          # in elements
COLS = (1, 15, 16, 17, 33)
NORMS = ((1.0, 0.0), (1.0 / 255.0, -0.5), (0.0078125, -1.0))

_plane = np.random.default_rng(2400).integers(0, 256, (ROWS, WIDTH), dtype=np.uint8)
_plane.reshape(-1)[:2] = (0, 255)
_plane.setflags(write=False)


def values(px, fmt, scale, bias):
    """The window's elements as the format's bytes, [rows, cols, elem]: numpy's float32 arithmetic, two roundings."""
    if fmt == 0:
        return np.ascontiguousarray(px).reshape(px.shape + (1,))
    v = px.astype(np.float32) * np.float32(scale) + np.float32(bias)
    if fmt == 1:
        v = v.astype(np.float16)
    elif fmt == 2:                                             # round to nearest even on the float32 bits, in integers
        u = np.ascontiguousarray(v).view(np.uint32).astype(np.uint64)
        v = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.ascontiguousarray(v).view(np.uint8).reshape(px.shape + (ELEM[fmt],))


def scatter(out, plane, window, fmt, scale, bias, pitch, step, offset, zero=False):
    """Element (r, c) of the window to byte offset + r * pitch + c * step of ``out``, and nothing else."""
    r0, r1, c0, c1 = window
    v = values(plane[r0:r1, c0:c1], fmt, scale, bias)
    if zero:
        v = np.zeros_like(v)
    e = ELEM[fmt]
    at = offset + np.arange(r1 - r0)[:, None, None] * pitch + np.arange(c1 - c0)[None, :, None] * step + np.arange(e)[None, None, :]
    out[at] = v
    return out


def needed(rows, cols, fmt, pitch, step):
    return (rows - 1) * pitch + (cols - 1) * step + ELEM[fmt]


def windows():
    return [(r0, r0 + rows, c0, c0 + cols) for cols in COLS for rows, r0 in ((1, 2), (3, 1)) for c0 in (0, 5, WIDTH - cols)]


@pytest.mark.parametrize("fmt", range(4))
@pytest.mark.parametrize("k", STEPS)
def test_strided_windows_match_a_numpy_scatter(pkg, fmt, k):
    e = ELEM[fmt]
    step = k * e
    for wi, window in enumerate(windows()):
        rows, cols = window[1] - window[0], window[3] - window[2]
        scale, bias = NORMS[0] if fmt == 0 else NORMS[wi % 3]
        for slack in (0, 3 * e):                               # a pitch of exactly the row's elements, and a larger one
            pitch = cols * step + slack
            for offset in range(0, 16, e):                     # every residue of 16 the format allows: no alignment rule applies
                out_bytes = offset + needed(rows, cols, fmt, pitch, step) + 21
                info = {}
                got = pkg.deliver_host(_plane, window, fmt, scale, bias, pitch=pitch, offset=offset, out_bytes=out_bytes, step=step, info=info)
                want = scatter(np.full(out_bytes, PATTERN, np.uint8), _plane, window, fmt, scale, bias, pitch, step, offset)
                assert np.array_equal(got, want), (fmt, k, window, slack, offset)
                assert (info["units"], info["chunks"]) == pkg.deliver_units(rows, cols, fmt, step=step) == (rows * ((cols + 15) // 16), 1)


@pytest.mark.parametrize("fmt", range(4))
def test_transposed_task(pkg, fmt):
    """pitch = one element, step = rows elements: the window arrives transposed, and fills its buffer exactly."""
    e = ELEM[fmt]
    scale, bias = NORMS[0] if fmt == 0 else NORMS[1]
    for window in ((1, 4, 3, 36), (0, 5, 0, 149), (2, 3, 7, 24), (0, 2, 0, 1)):
        rows, cols = window[1] - window[0], window[3] - window[2]
        if rows == 1:                                          # (one row: step == elem would be the contiguous task)
            continue
        got = pkg.deliver_host(_plane, window, fmt, scale, bias, pitch=e, step=rows * e)
        assert got.size == rows * cols * e
        want = values(_plane[window[0]:window[1], window[2]:window[3]], fmt, scale, bias).transpose(1, 0, 2).reshape(-1)
        assert np.array_equal(got, want), (fmt, window)


@pytest.mark.parametrize("fmt", range(4))
def test_zero_flag_and_gate(pkg, fmt):
    e = ELEM[fmt]
    window, step, offset = (1, 4, 3, 36), 3 * e, 5 * e
    pitch = 33 * step + 2 * e
    scale, bias = NORMS[0] if fmt == 0 else NORMS[1]
    out_bytes = offset + needed(3, 33, fmt, pitch, step) + 9
    blank = lambda: np.full(out_bytes, PATTERN, np.uint8)
    full = scatter(blank(), _plane, window, fmt, scale, bias, pitch, step, offset)
    zeros = scatter(blank(), _plane, window, fmt, scale, bias, pitch, step, offset, zero=True)
    assert not np.array_equal(full, zeros)
    call = lambda **kw: pkg.deliver_host(_plane, window, fmt, scale, bias, pitch=pitch, offset=offset, out_bytes=out_bytes, step=step, **kw)
    assert np.array_equal(call(zero=True), zeros)              # zero bytes in the elements, the pattern between them
    assert np.array_equal(call(), full) and np.array_equal(call(gate_status=1), full)
    for status in (0, 2, 3, -2, 7):                            # anything but done
        assert np.array_equal(call(gate_status=status), zeros), status


@pytest.mark.parametrize("fmt", range(4))
def test_three_tasks_interleave_into_one_frame(pkg, fmt):
    """Three planes as the colours of a rows x cols x 3 frame, each with its own normalisation: together the tasks fill every
    byte of the frame, and nothing beyond it."""
    lib = pkg.load_library()
    import ctypes as C
    e = ELEM[fmt]
    rng = np.random.default_rng(77 + fmt)
    for rows, cols in ((3, 33), (1, 17), (5, 149)):
        planes = [rng.integers(0, 256, (rows, cols), dtype=np.uint8) for _ in range(3)]
        norms = [NORMS[0]] * 3 if fmt == 0 else list(NORMS)
        frame_bytes = rows * cols * 3 * e
        raw = np.full(frame_bytes + 64 + 16, PATTERN, np.uint8)
        lead = (-raw.ctypes.data) % 16
        buf = raw[lead: lead + frame_bytes + 64]
        win = (C.c_int * 4)(0, rows, 0, cols)
        for ch in range(3):
            rc = lib.nblic_amd_debug_deliver_host_ex(planes[ch].ctypes.data, rows, cols, win, fmt, norms[ch][0], norms[ch][1], 0, -1, buf.ctypes.data, frame_bytes,
                                                     ch * e, cols * 3 * e, 3 * e, None, None)
            assert rc == 0
        want = np.stack([values(p, fmt, *nb) for p, nb in zip(planes, norms)], axis=2).reshape(-1)
        assert np.array_equal(buf[:frame_bytes], want), (fmt, rows, cols)
        assert (buf[frame_bytes:] == PATTERN).all() and (raw[:lead] == PATTERN).all()


def test_unit_and_chunk_counts(pkg):
    plane = np.random.default_rng(5).integers(0, 256, (300, 150), dtype=np.uint8)
    for fmt in range(4):
        e = ELEM[fmt]
        info = {}
        pkg.deliver_host(plane, (0, 300, 0, 150), fmt, step=3 * e, info=info)
        assert info == {"units": 300 * 10, "chunks": 3} and pkg.deliver_units(300, 150, fmt, step=3 * e) == (3000, 3)
        for cols, per_row in ((1, 1), (15, 1), (16, 1), (17, 2), (32, 2), (33, 3)):      # no head gap: sixteen pixels counted from col0
            info = {}
            pkg.deliver_host(plane, (7, 9, 3, 3 + cols), fmt, step=2 * e, offset=e, info=info)
            assert info["units"] == 2 * per_row == pkg.deliver_units(2, cols, fmt, step=2 * e)[0], (cols, fmt)
        # the element size as the step is the contiguous task, with its head gap
        assert pkg.deliver_units(300, 150, fmt, step=e) == pkg.deliver_units(300, 150, fmt)


def test_refusals(pkg):
    ok = dict(window=(1, 4, 3, 36), fmt=1, scale=0.5, bias=1.0, step=6, pitch=200, offset=2, out_bytes=2 + 2 * 200 + 32 * 6 + 2)
    pkg.deliver_host(_plane, **ok)
    pkg.deliver_host(_plane, **{**ok, "pitch": 2})             # a strided task may have any pitch from the element size up
    bad = [dict(step=7), dict(step=0), dict(step=1), dict(step=(1 << 20) + 2), dict(pitch=201), dict(pitch=0), dict(pitch=1), dict(pitch=(1 << 40) + 2),
           dict(offset=3, out_bytes=1000), dict(out_bytes=ok["out_bytes"] - 1), dict(offset=10 ** 6),
           dict(scale=float("nan")), dict(bias=float("inf")), dict(scale=float("-inf")), dict(bias=float("nan")),
           dict(fmt=0, scale=2.0, bias=0.0, step=3), dict(fmt=0, scale=1.0, bias=0.5, step=3), dict(fmt=4), dict(fmt=-1),
           dict(fmt=3, step=6, pitch=200, out_bytes=2000, offset=4), dict(fmt=3, step=8, pitch=202, out_bytes=2000, offset=4),
           dict(fmt=3, step=8, pitch=200, offset=2, out_bytes=2000),
           dict(window=(1, 1, 3, 36)), dict(window=(1, ROWS + 1, 3, 36)), dict(window=(1, 4, 117, 150)), dict(window=(-1, 4, 3, 36))]
    for change in bad:
        with pytest.raises(ValueError):
            pkg.deliver_host(_plane, **{**ok, **change})
    pkg.deliver_host(_plane, **{**ok, "fmt": 0, "scale": 1.0, "bias": 0.0, "step": 3})
    pkg.deliver_host(_plane, **{**ok, "fmt": 3, "step": 8, "pitch": 200, "offset": 4, "out_bytes": 2000})
    pkg.deliver_host(_plane, **{**ok, "step": 1 << 20, "pitch": 2, "out_bytes": 2 + 2 * 2 + 32 * (1 << 20) + 2})
    # step == elem keeps the contiguous rule: a pitch below the window's row is refused
    with pytest.raises(ValueError):
        pkg.deliver_host(_plane, **{**ok, "step": 2, "pitch": 64})


@pytest.mark.parametrize("fmt", range(4))
def test_element_size_as_the_step_is_the_old_hook(pkg, fmt):
    e = ELEM[fmt]
    scale, bias = NORMS[0] if fmt == 0 else NORMS[2]
    for window in ((1, 4, 3, 36), (0, 5, 0, 149), (2, 3, 7, 24), (4, 5, 148, 149)):
        rows, cols = window[1] - window[0], window[3] - window[2]
        for slack in (0, e, 3 * e):
            for offset in range(0, 16, e):
                kw = dict(pitch=cols * e + slack, offset=offset, out_bytes=offset + (rows - 1) * (cols * e + slack) + cols * e + 19)
                a, b = {}, {}
                old = pkg.deliver_host(_plane, window, fmt, scale, bias, info=a, **kw)
                new = pkg.deliver_host(_plane, window, fmt, scale, bias, step=e, info=b, **kw)
                assert np.array_equal(old, new) and a == b, (fmt, window, slack, offset)
