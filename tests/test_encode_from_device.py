"""GPU suite (-m gpu): encode from device memory.  The collect kernel on caller-made sources (nblic_amd_debug_collect) against
the host walk and numpy; the four _from calls on torch tensors in the layouts a producer has -- channels-last float16, an
interleaved uint8 frame, a crop of a pitched surface, bfloat16 and float32 lists -- byte for byte against the existing
calls on the collected planes, indexes and reconstructions included; sources used in place; sources and calls that are
refused; and the host calls on the same planes, which return what they returned before."""
import numpy as np
import pytest

from collect_inputs import ELEM, NORMS, all_patterns, as_values, element_bits, grid, lay_out

pytestmark = pytest.mark.gpu

DTYPES = ("uint8", "float16", "bfloat16", "float32")
SHAPES = ((33, 47), (64, 64), (1, 17), (40, 1))
MODES = ((0, 1), (2, 1), (0, 2), (1, 3))                       # (near, effort) of the mode call; effort 0 has a call of its own
GUARD = 256


def _torch():
    import torch
    return torch


def _values(t):
    """A 2-D device tensor's elements on the host, as collect_numpy takes them (bfloat16: the bit patterns)."""
    torch = _torch()
    host = t.contiguous().cpu()
    if host.dtype == torch.bfloat16:
        return host.view(torch.int16).numpy().view(np.uint16)
    return host.numpy()


def _planes(pkg, views, fmt, scale, bias):
    """The collected planes of device views: the library's host walk, which must agree with numpy."""
    _torch().cuda.synchronize()
    planes = []
    for v in views:
        vals = np.ascontiguousarray(_values(v))
        rows, cols = vals.shape
        host = pkg.collect_host(vals, fmt, scale, bias, rows=rows, cols=cols)
        assert np.array_equal(host, pkg.collect_numpy(vals, fmt, scale, bias))
        planes.append(np.ascontiguousarray(host))
    return planes


def _sources(shape, seed):
    """(name, list of 2-D device views, scale, bias) of every layout, for images of one shape."""
    torch = _torch()
    h, w = shape
    rng = np.random.default_rng(seed)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = []
    nchw = dev((rng.random((2, 3, h, w), np.float32) * 1.2 - 0.1).astype(np.float16)).contiguous(memory_format=torch.channels_last)
    out.append(("float16 channels-last", [nchw[n][c] for n in range(2) for c in range(3)], 255.0, 0.0, nchw))
    frame = dev(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    out.append(("interleaved uint8 frame", [frame[:, :, c] for c in range(3)], 1.0, 0.0, None))
    surface = dev(rng.integers(0, 256, (h + 3, w + 13), dtype=np.uint8))
    out.append(("crop of a pitched surface", [surface[2:2 + h, 5:5 + w], surface[1:1 + h, 7:7 + w]], 1.0, 0.0, None))
    bf = dev((rng.random((2, h, w + 2), np.float32) * 300 - 20)).to(torch.bfloat16)
    out.append(("bfloat16 list", [bf[0, :, 1:1 + w], bf[1, :, :w]], 1.0, 0.0, None))
    f32 = dev(rng.random((2, h + 1, w), np.float32) * 2 - 1)
    out.append(("float32 list", [f32[0, 1:], f32[1, :h]], 127.5, 127.5, None))
    return out


def test_kernel_on_caller_made_sources(gpu_ctx, pkg):
    """Hundreds of tasks of all four formats in ONE launch: sources at every element-aligned residue, every step and pitch of
    the CPU grid (thinned), every bit pattern of the half formats, tasks of more than one chunk and tasks of a pixel range."""
    tasks, bits_of = [], []
    for fmt in range(4):
        for k, t in enumerate(grid(fmt)):
            if k % 3:                                          # (the CPU grid, thinned: every residue still meets every layout)
                continue
            tasks.append(dict(raw=t["raw"][t["residue"]:], rows=t["rows"], cols=t["cols"], fmt=fmt, pitch=t["pitch"], step=t["step"],
                              scale=t["scale"], bias=t["bias"], base_offset=t["residue"] + 16 * (k % 15), residue=t["residue"], layout=t["layout"]))
            bits_of.append(t["bits"])
        assert {(t["residue"], t["layout"]) for t in tasks if t["fmt"] == fmt} == {(r, l) for r in range(0, 16, ELEM[fmt]) for l in range(4)}
    for fmt in (1, 2):
        for scale, bias in NORMS:
            bits = all_patterns(fmt)
            tasks.append(dict(raw=bits, rows=256, cols=256, fmt=fmt, scale=scale, bias=bias, base_offset=2 * len(tasks) % 256))
            bits_of.append(bits)
    rng = np.random.default_rng(1)
    for fmt, step, slack, rng_px in ((3, 1, 3, None), (0, 3, 1, None), (1, 1, 0, (129 * 7 + 5, 129 * 100)), (0, 1, 2, (4096, 16384)), (2, 2, 0, (16383, 0))):
        e = ELEM[fmt]
        bits = element_bits(rng, fmt, (130, 129))              # two chunks; rows end inside units
        pitch = (128 * step + 1 + slack) * e
        scale, bias = NORMS[0] if fmt == 0 else NORMS[1]
        tasks.append(dict(raw=lay_out(bits, fmt, pitch, step * e, 0), rows=130, cols=129, fmt=fmt, pitch=pitch, step=step * e, scale=scale, bias=bias,
                          base_offset=e * 3, **({"px_range": rng_px} if rng_px else {})))
        bits_of.append(bits)
    assert len(tasks) > 700 and pkg.collect_units(130, 129)[1] == 2
    live = pkg.live_resources()
    outs = gpu_ctx.debug_collect(tasks)
    assert pkg.live_resources() == live and len(outs) == len(tasks)
    for i, (t, bits, got) in enumerate(zip(tasks, bits_of, outs)):
        fmt, n = t["fmt"], t["rows"] * t["cols"]
        want = pkg.collect_numpy(as_values(bits, fmt), fmt, t["scale"], t["bias"]).reshape(-1)
        px0, px1 = t.get("px_range", (0, 0))
        px1 = px1 or n
        what = (i, {k: v for k, v in t.items() if k != "raw"})
        assert np.array_equal(got[GUARD + px0:GUARD + px1], want[px0:px1]), what
        assert (got[:GUARD + px0] == pkg.COLLECT_PATTERN).all() and (got[GUARD + px1:] == pkg.COLLECT_PATTERN).all(), what
        host = pkg.collect_host(t["raw"], fmt, t["scale"], t["bias"], pitch=t.get("pitch"), step=t.get("step"), rows=t["rows"], cols=t["cols"],
                                px_range=t.get("px_range"))
        assert np.array_equal(got[GUARD:GUARD + n], host.reshape(-1)), what
    sound = dict(raw=np.zeros(64, np.uint16), rows=4, cols=8, fmt=1, pitch=32, step=4)
    gpu_ctx.debug_collect([sound])
    for bad in (dict(raw=np.zeros(62, np.uint16)), dict(step=3), dict(step=1), dict(pitch=30 + 1), dict(base_offset=1), dict(base_offset=256), dict(rows=0),
                dict(scale=float("nan")), dict(fmt=0, scale=2.0), dict(px_range=(0, 33)), dict(fmt=4)):
        with pytest.raises(ValueError):
            gpu_ctx.debug_collect([sound, dict(sound, **bad)])


@pytest.mark.parametrize("shape", SHAPES)
def test_from_calls_match_the_parent_calls(gpu_ctx, pkg, shape):
    """Every layout x every mode, the indexed pair at every_rows 16 with band_rows 5 and 0: streams, indexes and host
    reconstructions equal what the existing calls return for the collected planes."""
    h, w = shape
    for name, views, scale, bias, whole in _sources(shape, 7 + h):
        fmt = pkg.collect_format(views[0].dtype)
        planes = _planes(pkg, views, fmt, scale, bias)
        m = len(views)
        # the mode call: every image in every NBLIC mode
        nears = [n for n, _ in MODES for _ in range(m)]
        efforts = [e for _, e in MODES for _ in range(m)]
        want, want_rec = gpu_ctx.encode_modes(planes * len(MODES), nears, efforts)
        info = {}
        got = gpu_ctx.encode_batch_from(views * len(MODES), scale=scale, bias=bias, near=nears, effort=efforts, info=info)
        assert info["rc"] == 0 and got == want, name
        assert all(np.array_equal(a, b) for a, b in zip(info["recons"], want_rec)), name
        assert gpu_ctx.encode_batch_from(views, scale=scale, bias=bias) == gpu_ctx.encode_batch(planes), name       # the defaults: -n0 -e1
        assert gpu_ctx.encode_batch_from(views, scale=scale, bias=bias, effort=0) == gpu_ctx.qencode_batch(planes), name
        for band_rows in (5, 0):
            assert gpu_ctx.encode_batch_from(views, scale=scale, bias=bias, every_rows=16, band_rows=band_rows) == \
                gpu_ctx.encode_batch_indexed(planes, 16, band_rows), (name, band_rows)
            assert gpu_ctx.encode_batch_from(views, scale=scale, bias=bias, effort=0, every_rows=16, band_rows=band_rows) == \
                gpu_ctx.qencode_batch_indexed(planes, 16, band_rows), (name, band_rows)
        if whole is not None:                                  # the [N, C, H, W] tensor as it is: every channel an image, n-major
            assert gpu_ctx.encode_batch_from(whole, scale=scale, bias=bias) == got[:m], name
            crop = gpu_ctx.encode_batch_from(whole, rows=(h // 2, 0), cols=(0, max(w - 1, 1)), scale=scale, bias=bias)
            assert crop == gpu_ctx.encode_batch([p[h // 2:, :max(w - 1, 1)] for p in planes]), name


def test_in_place_and_collected(gpu_ctx, pkg):
    torch = _torch()
    rng = np.random.default_rng(3)
    n, h, w = 4, 33, 47
    planes = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(n)]
    tensors = [torch.from_numpy(p).cuda() for p in planes]
    torch.cuda.synchronize()
    outs, lens = gpu_ctx.encode_ptrs([t.data_ptr() for t in tensors], [(h, w)] * n, True)
    want = [o[:int(k)].tobytes() for o, k in zip(outs, lens)]
    s0 = gpu_ctx.collect_stats()
    assert gpu_ctx.encode_batch_from(tensors) == want
    assert gpu_ctx.encode_batch_from(torch.stack(tensors)) == want             # one [N, H, W] tensor
    s1 = gpu_ctx.collect_stats()
    assert [b - a for a, b in zip(s0, s1)] == [2 * n, 0, 0, 0]                   # used where they lie: no kernel ran
    got = gpu_ctx.encode_batch_from(tensors, cols=(1, 0))                       # one column cropped: the pitch is no longer the width
    s2 = gpu_ctx.collect_stats()
    assert got == gpu_ctx.encode_batch([p[:, 1:] for p in planes])
    d = [b - a for a, b in zip(s1, s2)]
    assert d[0] == 0 and d[1] == n and d[3] == n * h * (w - 1) and 1 <= d[2] <= n // 2      # a launch per group, never per image
    pairs = gpu_ctx.encode_batch_from(tensors, cols=(1, 0), every_rows=8, band_rows=8)
    s3 = gpu_ctx.collect_stats()
    assert pairs == gpu_ctx.encode_batch_indexed([p[:, 1:] for p in planes], 8, 8)
    d = [b - a for a, b in zip(s2, s3)]
    assert d[0] == 0 and d[1] == n and d[3] == n * h * (w - 1) and 5 <= d[2] < 5 * n      # five bands an image: a launch per group step, never per image
    ms0, timed0 = gpu_ctx.collect_ms()
    gpu_ctx.enable_timing(True)
    try:
        assert gpu_ctx.encode_batch_from(tensors, cols=(1, 0)) == got
    finally:
        gpu_ctx.enable_timing(False)
    ms1, timed1 = gpu_ctx.collect_ms()
    assert timed1 - timed0 == gpu_ctx.collect_stats()[2] - s3[2] >= 1 and ms1 > ms0


def _allocation_end(t):
    """The end of the allocation a tensor lies in, as the caching allocator reports its segments."""
    torch = _torch()
    p = t.data_ptr()
    for seg in torch.cuda.memory_snapshot():
        if seg["address"] <= p < seg["address"] + seg["total_size"]:
            return seg["address"] + seg["total_size"]
    raise AssertionError("the tensor lies in no segment of the allocator")


def test_refused_sources_and_calls(gpu_ctx, pkg):
    torch = _torch()
    rng = np.random.default_rng(4)
    h, w = 20, 24
    t = torch.from_numpy(rng.random((3, h, w + 8), np.float32).astype(np.float16)).cuda()
    views = [t[k, :, 3:3 + w] for k in range(3)]
    planes = _planes(pkg, views, 1, 255.0, 0.0)
    sound, fmt = pkg._srcs_of(views, None, None)
    assert fmt == 1
    want = gpu_ctx.encode_from_srcs(sound, 1, 255.0)
    assert want == gpu_ctx.encode_batch(planes)
    ptr, pitch, step, cap, _, _ = sound[1]
    extent = (h - 1) * pitch + (w - 1) * step + 2
    host = np.zeros((h, w), np.float16)
    end = _allocation_end(t)
    bad = {"a host pointer": (host.ctypes.data, w * 2, 2, host.nbytes, h, w),
           "a pointer off by one byte": (ptr + 1, pitch, step, cap - 1, h, w),
           "a cap one byte short": (ptr, pitch, step, extent - 1, h, w),
           "an extent past the end of the allocation": (end - 64, 128, 2, 1 << 20, 1, 33),
           "a zero-row image": (ptr, pitch, step, cap, 0, w),
           "a step below the element size": (ptr, pitch, 1, cap, h, w),
           "a pitch that is no multiple": (ptr, pitch + 1, step, cap, h, w),
           "a width the encoder does not take": (ptr, pitch, step, 1 << 40, h, 65536)}
    srcs = [sound[0]]
    for d in bad.values():
        srcs += [d, sound[len(srcs) % 3]]
    assert gpu_ctx.encode_from_srcs([(ptr, pitch, step, extent, h, w)], 1, 255.0) == [want[1]]           # (the cap that just holds it)
    assert gpu_ctx.encode_from_srcs([(end - 64, 128, 2, 1 << 20, 1, 32)], 1, 255.0)[0] is not None      # (the row that just ends with the allocation)
    for kw in (dict(), dict(effort=0), dict(every_rows=8), dict(effort=0, every_rows=8, band_rows=4)):
        info = {}
        got = gpu_ctx.encode_from_srcs(srcs, 1, 255.0, info=info, **kw)
        alone = gpu_ctx.encode_from_srcs([s for k, s in enumerate(srcs) if k % 2 == 0], 1, 255.0, **kw)
        assert info["rc"] != 0
        for k, g in enumerate(got):
            if k % 2:
                assert g is None or g == (None, None), (list(bad)[k // 2], kw)
            else:
                assert g == alone[k // 2] and g is not None and (g[0] if isinstance(g, tuple) else g), (k, kw)
    # the whole call refused: nothing launched, nothing counted
    u8 = torch.from_numpy(rng.integers(0, 256, (h, w + 1), dtype=np.uint8)).cuda()[:, 1:]
    s0 = gpu_ctx.collect_stats()
    for view, kw in ((u8, dict(scale=2.0)), (u8, dict(bias=1.0)), (views[0], dict(scale=float("nan"))), (views[0], dict(bias=float("inf"))),
                     (views[0], dict(scale=float("nan"), effort=0)), (u8, dict(scale=2.0, every_rows=8)), (u8, dict(scale=2.0, every_rows=8, effort=0))):
        with pytest.raises(ValueError):
            gpu_ctx.encode_batch_from([view], **kw)
    with pytest.raises(ValueError):
        gpu_ctx.encode_from_srcs(sound, 4, 1.0)
    assert gpu_ctx.collect_stats() == s0
    with pytest.raises(ValueError):
        gpu_ctx.encode_batch_from([views[0], u8])              # one dtype per call
    with pytest.raises(ValueError):
        gpu_ctx.encode_batch_from(views, effort=[0, 1, 1])     # effort 0 takes a whole call
    with pytest.raises(ValueError):
        gpu_ctx.encode_batch_from(views, near=1, every_rows=8)
    assert gpu_ctx.encode_from_srcs(sound, 1, 255.0) == want


def test_nothing_else_moved(gpu_ctx, pkg):
    """Host planes, device planes and sources through the same groups, one after the other and again: the same bytes."""
    torch = _torch()
    rng = np.random.default_rng(6)
    planes = [rng.integers(0, 256, (33, 47), dtype=np.uint8) for _ in range(5)] + [rng.integers(0, 256, (64, 64), dtype=np.uint8)]
    nears, efforts = [0, 2, 0, 1, 0, 3], [1, 1, 2, 3, 1, 2]
    before = (gpu_ctx.encode_batch(planes), gpu_ctx.encode_modes(planes, nears, efforts)[0], gpu_ctx.qencode_batch_indexed(planes, 16, 5))
    f = [torch.from_numpy((p.astype(np.float32) / 255).astype(np.float16)).cuda() for p in planes]
    frames = [torch.from_numpy(np.stack([p, p, p], -1)).cuda() for p in planes]
    dev = [torch.from_numpy(p).cuda() for p in planes]
    torch.cuda.synchronize()
    from_f16 = gpu_ctx.encode_batch_from(f, scale=255.0)
    assert from_f16 == before[0]                               # (k / 255 in float16, times 255, rounds back to k)
    assert gpu_ctx.encode_batch_from([fr[:, :, 1] for fr in frames], near=nears, effort=efforts) == before[1]
    assert gpu_ctx.encode_batch_from(dev + [fr[:, :, 2] for fr in frames], effort=0, every_rows=16, band_rows=5) == before[2] + before[2]
    outs, lens = gpu_ctx.encode_ptrs([t.data_ptr() for t in dev], [p.shape for p in planes], True)
    assert [o[:int(k)].tobytes() for o, k in zip(outs, lens)] == before[0]
    after = (gpu_ctx.encode_batch(planes), gpu_ctx.encode_modes(planes, nears, efforts)[0], gpu_ctx.qencode_batch_indexed(planes, 16, 5))
    assert after == before
    for s, p in zip(from_f16, planes):
        assert np.array_equal(gpu_ctx.decode_batch([s])[0][0], p)
