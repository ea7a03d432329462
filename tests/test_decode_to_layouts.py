"""GPU suite (-m gpu): decode to ANY device layout.  The delivery kernel's strided path on caller-made planes
(nblic_amd_debug_deliver_ex) against the host walk, byte for byte; then nblic_amd_decode_batch_to_ex and
nblic_amd_decode_batch_indexed_to_ex through ``layout="any"``: the three streams of a frame into a uint8 [N, H, W, 3] batch
and into a channels-last float16 tensor with a scale and bias per channel, against the numpy expression on the planes that
``decode_batch`` returns, bit for bit; padding that keeps its pattern; a stream that fails and destinations that are refused,
each costing its own channel only."""
import numpy as np
import pytest

import inputs
from test_decode_to_device import _bits, _elements, _filled
from test_deliver_strided_host import ELEM, NORMS, PATTERN
from test_indexed_batch_decode import _live

pytestmark = pytest.mark.gpu

GEOMS = ((9, 23, 3), (33, 70, 7))                             # height, width and the R of the frame's seek indexes
CLASSES = (("n", 0, 1), ("n", 2, 1), ("n", 0, 2), ("q", 0, 0))
CHANNEL_NORMS = ((1.0 / 255.0, -0.5), (0.0078125, -1.0), (2.0 / 255.0, 0.25))     # three different scale / bias pairs
FRAMES = 2

_cache = {}


@pytest.fixture(scope="module")
def ctx(pkg, gpu_ctx):
    """A context of this module's own (made after the session's, which initialises torch first), so that the session's
    context reaches the later modules in the state the earlier ones left it in."""
    c = pkg.Context(device=0, n_slots=3, n_coders=3)
    yield c
    c.close()


def _torch():
    import torch
    return torch


def _frames(ctx, oracle, h, w, R):
    """FRAMES x 3 (stream, index), n-major, the classes rotating over the streams; and decode_batch's planes of them."""
    key = (h, w, R)
    if key not in _cache:
        pairs = []
        for k in range(FRAMES * 3):
            kind, near, effort = CLASSES[(k + (h % 4)) % 4]
            img = inputs.syn1(h, w, 40 + k)
            s = oracle.qencode(img) if kind == "q" else oracle.encode(img, near, effort)[0]
            pairs.append((s, ctx.build_index(s, R)))
        planes = [p[0] for p in ctx.decode_batch([s for s, _ in pairs])]
        assert all(p is not None and p.shape == (h, w) for p in planes)
        _cache[key] = (pairs, planes)
    return _cache[key]


def _decode(ctx, how, pairs, out, **kw):
    if how == "indexed":
        return ctx.decode_batch_indexed_into(pairs, out, layout="any", **kw)
    return ctx.decode_batch_into([s for s, _ in pairs], out, layout="any", **kw)


def test_classes_cover_the_four(ctx, oracle):
    seen = set()
    for h, w, R in GEOMS:
        seen |= {CLASSES[(k + (h % 4)) % 4] for k in range(FRAMES * 3)}
    assert seen == set(CLASSES)


def test_strided_kernel_matches_the_host_walk(ctx, pkg):
    """Contiguous and strided tasks of all four formats mixed in ONE launch: every step and column count of the CPU grid,
    the wave's edge (63, 64, 65 columns), a 70 x 149 window and a task of three chunks with a partial last one, transposed
    tasks, zero flags and gates.  Every buffer equals the host walk's, pattern bytes included."""
    rng = np.random.default_rng(24)
    small = rng.integers(0, 256, (5, 149), dtype=np.uint8)
    tall = rng.integers(0, 256, (70, 149), dtype=np.uint8)
    big = rng.integers(0, 256, (300, 150), dtype=np.uint8)
    tasks, k = [], 0
    for fmt in range(4):
        e = ELEM[fmt]
        for steps in (2, 3, 4, 7):
            for cols in (1, 15, 16, 17, 33, 63, 64, 65):
                for rows, r0 in ((1, 2), (3, 1)):
                    c0 = (0, 5, 149 - cols)[k % 3]
                    scale, bias = NORMS[0] if fmt == 0 else NORMS[k % 3]
                    step, offset = steps * e, (k * e) % 16
                    pitch = cols * step + (0, 3 * e)[k % 2]
                    need = (rows - 1) * pitch + (cols - 1) * step + e
                    tasks.append(dict(plane=small, window=(r0, r0 + rows, c0, c0 + cols), fmt=fmt, scale=scale, bias=bias, step=step, pitch=pitch, offset=offset,
                                      out_bytes=offset + need + 21, base_offset=k % 16))
                    if k % 4 == 0:                             # a contiguous task between them
                        tasks.append(dict(plane=small, window=(r0, r0 + rows, c0, c0 + cols), fmt=fmt, scale=scale, bias=bias, offset=offset,
                                          out_bytes=offset + (rows - 1) * cols * e + cols * e + 21, base_offset=(k + 3) % 16))
                    k += 1
        nb = NORMS[0] if fmt == 0 else NORMS[1]
        tasks.append(dict(plane=tall, window=(0, 70, 0, 149), fmt=fmt, scale=nb[0], bias=nb[1], step=3 * e, offset=e, base_offset=fmt + 1))
        tasks.append(dict(plane=big, window=(0, 300, 0, 150), fmt=fmt, scale=nb[0], bias=nb[1], step=3 * e, pitch=150 * 3 * e + e, offset=2 * e, base_offset=5 + fmt))
        tasks.append(dict(plane=big, window=(0, 300, 0, 150), fmt=fmt, scale=nb[0], bias=nb[1], offset=e, base_offset=fmt))
        tasks.append(dict(plane=small, window=(1, 4, 3, 36), fmt=fmt, scale=nb[0], bias=nb[1], step=3 * e, pitch=e, offset=0))            # transposed
        tasks.append(dict(plane=tall, window=(0, 70, 0, 149), fmt=fmt, scale=nb[0], bias=nb[1], step=70 * e, pitch=e, offset=3 * e))       # transposed
        for status in (1, 0, 2, -7):
            tasks.append(dict(plane=small, window=(1, 4, 3, 36), fmt=fmt, scale=nb[0], bias=nb[1], step=3 * e, pitch=100 * e, offset=e, gate_status=status))
        tasks.append(dict(plane=small, window=(0, 5, 0, 149), fmt=fmt, step=2 * e, offset=7 * e, zero=True))
    assert pkg.deliver_units(300, 150, 0, step=3) == (3000, 3) and pkg.deliver_units(70, 149, 0, step=3) == (700, 1)
    strided = sum(1 for t in tasks if "step" in t)
    assert strided > 250 and len(tasks) - strided > 60
    with _live(pkg):
        outs = ctx.debug_deliver(tasks)
    assert ctx.deliver_stats() == (len(tasks), strided)
    for i, (t, got) in enumerate(zip(tasks, outs)):
        host = pkg.deliver_host(t["plane"], t["window"], t["fmt"], t.get("scale", 1.0), t.get("bias", 0.0), pitch=t.get("pitch"), offset=t.get("offset", 0),
                                out_bytes=got.size, zero=t.get("zero", False), gate_status=t.get("gate_status", -1), step=t.get("step"))
        assert np.array_equal(got, host), (i, {k: v for k, v in t.items() if k != "plane"})
    for bad in (dict(step=0), dict(step=5, fmt=1), dict(step=(1 << 20) + 1), dict(step=3, out_bytes=3 * 149 * 5 - 3)):
        with pytest.raises(ValueError):
            ctx.debug_deliver([dict(plane=small, window=(0, 5, 0, 149), fmt=0, step=3), dict(dict(plane=small, window=(0, 5, 0, 149), fmt=0), **bad)])


@pytest.mark.parametrize("how", ("indexed", "plain"))
def test_uint8_nhwc_batch(ctx, pkg, oracle, how):
    """The three streams of every frame into a uint8 [N, H, W, 3] tensor, handed over as its permute(0, 3, 1, 2)."""
    for h, w, R in GEOMS:
        pairs, planes = _frames(ctx, oracle, h, w, R)
        out = _filled((FRAMES, h, w, 3), 0)
        with pytest.raises(ValueError):                        # layout="rows" still refuses the tensor
            ctx.decode_batch_into([s for s, _ in pairs], out.permute(0, 3, 1, 2))
        with pytest.raises(ValueError):
            ctx.decode_batch_indexed_into(pairs, [out[n, :, :, c] for n in range(FRAMES) for c in range(3)], layout="rows")
        assert bool((out == PATTERN).all())
        info = {}
        if how == "plain":                                     # (the context's grow-only task buffer exists from here on)
            assert _decode(ctx, how, pairs, _filled((FRAMES, h, w, 3), 0).permute(0, 3, 1, 2)) == [0] * len(pairs)
        with _live(pkg):
            assert _decode(ctx, how, pairs, out.permute(0, 3, 1, 2), info=info) == [0] * len(pairs) and info["rc"] == 0
        assert ctx.deliver_stats() == (len(pairs), len(pairs))
        want = np.stack(planes).reshape(FRAMES, 3, h, w).transpose(0, 2, 3, 1)
        assert np.array_equal(_bits(out), want), (how, h, w)


@pytest.mark.parametrize("how", ("indexed", "plain"))
def test_channels_last_float16_with_a_norm_per_channel(ctx, pkg, oracle, how):
    torch = _torch()
    for h, w, R in GEOMS:
        pairs, planes = _frames(ctx, oracle, h, w, R)
        out = _filled((FRAMES, h, w, 3), 1).permute(0, 3, 1, 2)
        assert out.is_contiguous(memory_format=torch.channels_last) and tuple(out.shape) == (FRAMES, 3, h, w)
        scales = [CHANNEL_NORMS[c][0] for _ in range(FRAMES) for c in range(3)]
        biases = [CHANNEL_NORMS[c][1] for _ in range(FRAMES) for c in range(3)]
        assert _decode(ctx, how, pairs, out, scale=scales, bias=biases) == [0] * len(pairs)
        got = _bits(out)
        for k, plane in enumerate(planes):
            assert np.array_equal(got[k // 3, k % 3], _elements(plane, 1, *CHANNEL_NORMS[k % 3])), (how, h, w, k)
        assert len({got[0, c].tobytes() for c in range(3)}) == 3
        # a window of rows and columns of the same, into a tensor of the window's shape
        r, c = (2, h - 1), (5, w - 3)
        win = _filled((FRAMES, r[1] - r[0], c[1] - c[0], 3), 1).permute(0, 3, 1, 2)
        assert _decode(ctx, how, pairs, win, rows=r, cols=c, scale=scales, bias=biases) == [0] * len(pairs)
        got = _bits(win)
        for k, plane in enumerate(planes):
            assert np.array_equal(got[k // 3, k % 3], _elements(plane[r[0]:r[1], c[0]:c[1]], 1, *CHANNEL_NORMS[k % 3])), (how, h, w, k)
        # one scale for every image, and scale / bias per image with layout="rows" on planar tensors
        flat = _filled((len(pairs), h, w), 1)
        assert _decode(ctx, how, pairs, flat, scale=CHANNEL_NORMS[0][0], bias=CHANNEL_NORMS[0][1]) == [0] * len(pairs)
        rows_layout = _filled((len(pairs), h, w), 1)
        call = ctx.decode_batch_indexed_into if how == "indexed" else ctx.decode_batch_into
        assert call(pairs if how == "indexed" else [s for s, _ in pairs], rows_layout, scale=scales, bias=biases) == [0] * len(pairs)
        assert ctx.deliver_stats() == (len(pairs), 0)
        for k, plane in enumerate(planes):
            assert np.array_equal(_bits(flat[k]), _elements(plane, 1, *CHANNEL_NORMS[0])), k
            assert np.array_equal(_bits(rows_layout[k]), _elements(plane, 1, *CHANNEL_NORMS[k % 3])), k


@pytest.mark.parametrize("fmt", (0, 3))
def test_padding_after_the_channel_keeps_its_pattern(ctx, pkg, oracle, fmt):
    h, w, R = GEOMS[1]
    pairs, planes = _frames(ctx, oracle, h, w, R)
    out = _filled((FRAMES, h, w, 4), fmt)
    norm = (1.0, 0.0) if fmt == 0 else CHANNEL_NORMS[1]
    assert ctx.decode_batch_into([s for s, _ in pairs], out[..., :3].permute(0, 3, 1, 2), layout="any", scale=norm[0], bias=norm[1]) == [0] * len(pairs)
    got = _bits(out)
    fill = int.from_bytes(bytes([PATTERN]) * ELEM[fmt], "little")
    assert (got[..., 3] == fill).all()
    for k, plane in enumerate(planes):
        assert np.array_equal(got[k // 3, :, :, k % 3], _elements(plane, fmt, *norm)), k


def test_a_failed_stream_and_refused_destinations_cost_their_own_channel(ctx, pkg, oracle):
    torch = _torch()
    h, w, R = GEOMS[1]
    pairs, planes = _frames(ctx, oracle, h, w, R)
    streams = [s for s, _ in pairs]
    norm = CHANNEL_NORMS[0]
    assert ctx.decode_batch_into(streams, _filled((FRAMES, h, w, 3), 0).permute(0, 3, 1, 2), layout="any") == [0] * 6      # (the grow-only task buffer)
    with _live(pkg):
        # a stream cut short in its payload fails on the device: zeros in ITS channel, the neighbours are right
        cut = list(streams)
        cut[4] = streams[4][:len(streams[4]) * 2 // 3]
        assert ctx.decode_batch([cut[4]])[0] is None
        out = _filled((FRAMES, h, w, 3), 1)
        info = {}
        status = ctx.decode_batch_into(cut, out.permute(0, 3, 1, 2), layout="any", scale=norm[0], bias=norm[1], info=info)
        assert status == [0, 0, 0, 0, -1, 0] and info["rc"] == -1
        got = _bits(out)
        for k, plane in enumerate(planes):
            want = np.zeros((h, w), np.uint16) if k == 4 else _elements(plane, 1, *norm)
            assert np.array_equal(got[k // 3, :, :, k % 3], want), k
        # a host tensor, a view that is too small, a scale that is not finite: each refused alone, nothing of it written
        for what in ("host", "small", "scale"):
            out = _filled((FRAMES, h, w, 3), 1)
            views = [out[n, :, :, c] for n in range(FRAMES) for c in range(3)]
            scales = [norm[0]] * 6
            cpu = None
            if what == "host":
                cpu = torch.from_numpy(np.full((h, w, 3 * 2), PATTERN, np.uint8)).view(torch.float16)
                views[1] = cpu[:, :, 1]
            elif what == "small":
                views[1] = out[0, :h - 1, :, 1]
            else:
                scales[1] = float("inf")
            for how in ("indexed", "plain"):
                info = {}
                assert _decode(ctx, how, pairs, views, scale=scales, bias=norm[1], info=info) == [0, -1, 0, 0, 0, 0] and info["rc"] == -1, (what, how)
                got = _bits(out)
                fill = int.from_bytes(bytes([PATTERN]) * 2, "little")
                for k, plane in enumerate(planes):
                    want = np.full((h, w), fill, np.uint16) if k == 1 else _elements(plane, 1, *norm)
                    assert np.array_equal(got[k // 3, :, :, k % 3], want), (what, how, k)
                assert ctx.deliver_stats() == (5, 5)
                if cpu is not None:
                    assert bool((cpu.view(torch.uint8) == PATTERN).all())
        # the raw call: a step that is no multiple of the element, a step beyond the limit, a window the capacity does not hold
        out = _filled((1, h, w, 3), 1)
        ptr, e = out.data_ptr(), 2
        sound = (ptr, w * 3 * e, 3 * e, out.numel() * e, 0, 0, 0, 0, norm[0], norm[1])
        assert ctx.decode_batch_to_ex(streams[:1], [sound], 1) == [0]
        for bad in ((ptr, w * 3 * e, 3, out.numel() * e), (ptr, w * 3 * e, (1 << 20) + 2, 1 << 40), (ptr, w * 3 * e + 1, 3 * e, out.numel() * e),
                    (ptr + 1, w * 3 * e, 3 * e, out.numel() * e), (ptr, w * 3 * e, 3 * e, (h - 1) * w * 3 * e + (w - 1) * 3 * e + e - 1),
                    (ptr, w * 3 * e, 3 * e + 2, out.numel() * e), (ptr, (1 << 40) + 2, 3 * e, 1 << 62), (ptr, 0, 3 * e, out.numel() * e)):
            fresh = _filled((1, h, w, 3), 1)
            moved = (fresh.data_ptr() + (bad[0] - ptr),) + bad[1:]
            assert ctx.decode_batch_to_ex(streams[:1], [moved + (0, 0, 0, 0, norm[0], norm[1])], 1) == [-1], bad
            assert ctx.decode_batch_indexed_to_ex(pairs[:1], [moved + (0, 0, 0, 0, norm[0], norm[1])], 1) == [-1], bad
            assert bool((fresh.view(torch.uint8) == PATTERN).all()), bad
        u8 = _filled((1, h, w, 3), 0)
        assert ctx.decode_batch_to_ex(streams[:1], [(u8.data_ptr(), w * 3, 3, u8.numel(), 0, 0, 0, 0, 2.0, 0.0)], 0) == [-1]
        assert ctx.decode_batch_to_ex(streams[:1], [(u8.data_ptr(), w * 3, 3, u8.numel(), 0, 0, 0, 0, 1.0, 0.5)], 0) == [-1]
        assert bool((u8 == PATTERN).all())
        assert ctx.decode_batch_to_ex(streams[:1], [sound], 4) == [-1] and ctx.decode_batch_indexed_to_ex(pairs[:1], [sound], -1) == [-1]
        # a transposed view works: a strided destination may have any pitch
        t = _filled((w, h), 0)
        assert ctx.decode_batch_into(streams[:1], [t.t()], layout="any") == [0]
        assert np.array_equal(_bits(t), planes[0].T)
