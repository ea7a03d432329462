"""CPU suite: the collect kernel's unit walk and arithmetic on the host (csrc/collect.h through nblic_amd_debug_collect_host)
against the numpy expression of the collected plane, bit for bit: every width, height, source residue, step and pitch of the
grid with NaN in every gap, every bit pattern of float16 and bfloat16, float32 around every tie, and the refusals."""
import numpy as np
import pytest

from collect_inputs import ELEM, GAP, NORMS, all_patterns, as_values, f32_bits, grid, lay_out


def _host(pkg, t, **kw):
    return pkg.collect_host(t["raw"], t["fmt"], t["scale"], t["bias"], pitch=t["pitch"], step=t["step"], offset=t["residue"],
                            rows=t["rows"], cols=t["cols"], **kw)


@pytest.mark.parametrize("fmt", range(4))
def test_grid_matches_numpy(pkg, fmt):
    """Widths 1, 15, 16, 17, 33 x heights 1, 2, 3 x every element-aligned residue modulo 16 x steps of 1, 3 and 4 elements
    with slack in the pitch, and transposed.  The gaps hold NaN (255 as a pixel): read as data they would show."""
    seen = set()
    for t in grid(fmt):
        want = pkg.collect_numpy(as_values(t["bits"], fmt), fmt, t["scale"], t["bias"])
        info = {}
        got = _host(pkg, t, info=info)
        assert np.array_equal(got, want), {k: v for k, v in t.items() if k not in ("raw", "bits")}
        n = t["rows"] * t["cols"]
        assert (info["units"], info["chunks"]) == pkg.collect_units(t["rows"], t["cols"]) == ((n + 15) // 16, 1)
        seen.add((t["cols"], t["rows"], t["residue"], t["layout"]))
    assert len(seen) == 5 * 3 * (16 // ELEM[fmt]) * 4


@pytest.mark.parametrize("fmt", range(4))
def test_pixel_ranges(pkg, fmt):
    """A task that writes the pixels [px0, px1) alone -- a band of an indexed batch -- leaves every other byte as it was."""
    t = next(g for g in grid(fmt) if g["cols"] == 33 and g["rows"] == 3 and g["step"] == 3 * ELEM[fmt])
    want = pkg.collect_numpy(as_values(t["bits"], fmt), fmt, t["scale"], t["bias"]).reshape(-1)
    for px0, px1 in ((0, 33), (33, 99), (17, 18), (15, 17), (16, 32), (1, 98), (66, 0)):
        info = {}
        got = _host(pkg, t, px_range=(px0, px1), info=info).reshape(-1)
        px1 = px1 or 99
        assert np.array_equal(got[px0:px1], want[px0:px1]) and (got[:px0] == pkg.COLLECT_PATTERN).all() and (got[px1:] == pkg.COLLECT_PATTERN).all()
        assert (info["units"], info["chunks"]) == pkg.collect_units(3, 33, px0, px1) == ((px1 + 15) // 16 - px0 // 16, 1)
    for bad in ((0, 100), (50, 50), (60, 40), (-1, 5)):
        with pytest.raises(ValueError):
            _host(pkg, t, px_range=bad)


@pytest.mark.parametrize("fmt", (1, 2))
@pytest.mark.parametrize("scale,bias", NORMS)
def test_every_pattern_of_the_half_formats(pkg, fmt, scale, bias):
    """All 65,536 bit patterns of float16 and of bfloat16 as one 256 x 256 image."""
    bits = all_patterns(fmt)
    want = pkg.collect_numpy(as_values(bits, fmt), fmt, scale, bias)
    info = {}
    got = pkg.collect_host(bits, fmt, scale, bias, rows=256, cols=256, info=info)
    assert np.array_equal(got, want)
    assert (info["units"], info["chunks"]) == (4096, 4)
    if (scale, bias) == (255.0, 0.0) and fmt == 1:             # a spot check of the numpy expression itself
        assert want[0x3C, 0x00] == 255 and want[0x38, 0x00] == 128 and want[0xBC, 0x00] == 0 and want[0x7E, 0x00] == 0


def test_float32_values(pkg):
    ties = np.arange(256, dtype=np.float32) + np.float32(0.5)
    around = np.concatenate([np.nextafter(ties, np.float32(-1)), ties, np.nextafter(ties, np.float32(1e9))]).astype(np.float32)
    listed = np.array([0.5, 1.5, 2.5, 254.5, 255.5, 0.0, -0.0, np.inf, -np.inf], np.float32)
    got = pkg.collect_host(listed.reshape(1, -1), 3)
    assert got.reshape(-1).tolist() == [0, 2, 2, 254, 255, 0, 0, 255, 0]
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32)
    assert not pkg.collect_host(nans.reshape(1, -1), 3, rows=1, cols=4).any()
    sub = np.array([0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000], np.uint32).view(np.float32)
    big = np.array([3e38, -3e38], np.float32)
    for values, scale, bias in ((around, 1.0, 0.0), (around, 0.5, 0.25), (around / np.float32(255), 255.0, 0.0), (listed, 127.5, 127.5),
                                (sub, 1.0, 0.0), (sub, 3e38, 0.0), (sub, 3e38, 0.5), (big, 2.0, 0.0), (big, 3e38, 0.0), (big, -2.0, 1.0), (big, 1.0, 0.0)):
        v = np.ascontiguousarray(values, np.float32).reshape(1, -1)
        want = pkg.collect_numpy(v, 3, scale, bias)
        assert np.array_equal(pkg.collect_host(v, 3, scale, bias), want), (scale, bias)
    assert pkg.collect_numpy(big.reshape(1, 2), 3, 2.0, 0.0).tolist() == [[255, 0]]
    k = pkg.collect_numpy(around.reshape(1, -1), 3)
    assert k[0, :256].tolist() == list(range(256)) and k[0, 512:].tolist() == [min(i + 1, 255) for i in range(256)]
    assert k[0, 256:512].tolist() == [min(i + (i & 1), 255) for i in range(256)]         # ties go to even


def test_views_with_strides(pkg):
    """A 2-D numpy view says its own pitch and step: a channel of an interleaved frame, a transposed plane, a crop."""
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (9, 21, 3), dtype=np.uint8)
    for c in range(3):
        assert np.array_equal(pkg.collect_host(frame[:, :, c], 0), frame[:, :, c])
    assert np.array_equal(pkg.collect_host(frame[:, :, 1].T, 0), frame[:, :, 1].T)
    f = rng.random((7, 40), np.float32)
    assert np.array_equal(pkg.collect_host(f[2:6, 3:36], 3, 255.0), pkg.collect_numpy(f[2:6, 3:36], 3, 255.0))
    h = f.astype(np.float16)
    assert np.array_equal(pkg.collect_host(h[::2, 1::3], 1, 255.0), pkg.collect_numpy(h[::2, 1::3], 1, 255.0))
    with pytest.raises(ValueError):
        pkg.collect_host(frame[::-1, :, 0], 0)


def test_refusals(pkg):
    """Each descriptor is sound except for the one field."""
    raw = lay_out(np.zeros((4, 8), np.uint16), 1, 64, 4, 2)
    sound = dict(fmt=1, scale=255.0, bias=0.0, pitch=64, step=4, offset=2, rows=4, cols=8)
    cap = 3 * 64 + 7 * 4 + 2
    assert raw.size == 2 + cap

    def refused(**kw):
        a = dict(sound, **kw)
        fmt, scale, bias = a.pop("fmt"), a.pop("scale"), a.pop("bias")
        try:
            pkg.collect_host(raw, fmt, scale, bias, **a)
        except ValueError:
            return True
        return False

    assert not refused() and not refused(cap=cap)
    assert refused(cap=cap - 1)                                # one byte short
    assert refused(rows=0) and refused(cols=0) and refused(rows=65536, cap=1 << 40) and refused(cols=65536, cap=1 << 40)
    assert refused(offset=3)                                   # the pointer is no multiple of the element size
    assert refused(pitch=63, cap=1 << 20) and refused(step=3, cap=1 << 20)
    assert refused(step=0) and refused(step=1) and refused(pitch=0) and refused(pitch=1)       # below the element size
    assert refused(step=(1 << 20) + 2, cap=1 << 40) and not refused(step=1 << 20, cap=1 << 40, rows=1, cols=1)
    assert refused(pitch=(1 << 40) + 2, cap=1 << 62) and not refused(pitch=1 << 40, cap=1 << 62, rows=1, cols=1)
    assert refused(fmt=4) and refused(fmt=-1)
    assert refused(scale=float("nan")) and refused(bias=float("inf")) and refused(scale=float("-inf"))
    assert refused(fmt=0, scale=255.0) and refused(fmt=0, scale=1.0, bias=1.0) and not refused(fmt=0, scale=1.0)
    assert [pkg.collect_format(n) for n in ("uint8", "torch.float16", np.dtype("float32"), "torch.bfloat16")] == [0, 1, 3, 2]
    with pytest.raises(ValueError):
        pkg.collect_format("float64")
    assert bytes(raw[:2]) == bytes([GAP, GAP]) and f32_bits([1.0])[0] == 0x3F800000
