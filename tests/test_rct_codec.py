"""GPU suite (-m gpu): colour frames through the public calls.  ``encode_batch_from(..., color="rct")`` in every effort and
through both indexed calls, byte for byte against the same call without the flag on the numpy-transformed planes and
against the oracle; ``decode_batch_into`` and ``decode_batch_indexed_into`` with ``color="rct"`` into uint8 NHWC and
channels-last float16 with a mean and std per channel, bit for bit against the original frame; frames that are refused or
fail as a whole next to frames that are complete; and the calls without ``color``, which return what they returned."""
import contextlib

import numpy as np
import pytest

import inputs
from rct_inputs import CHANNEL_NORMS, exhaustive_frame
from test_decode_to_device import _bits, _elements, _filled
from test_deliver_strided_host import PATTERN
from test_indexed_batch_decode import _forge, _live

pytestmark = pytest.mark.gpu

GEOMS = ((48, 80), (33, 17), (256, 256))                       # the last one: the exhaustive frame
LAYOUTS = ("nchw uint8", "nhwc uint8", "channels-last float16")
EVERY = 16

_cache = {}


@pytest.fixture(scope="module")
def ctx(pkg, gpu_ctx):
    """A context of this module's own (made after the session's, which initialises torch first)."""
    c = pkg.Context(device=0, n_slots=3, n_coders=3)
    yield c
    c.close()


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _frames(h, w):
    """[F, 3, h, w] uint8: channels that share a SYN-1 plane and differ by a quarter of a plane of their own seed."""
    if (h, w) == (256, 256):
        return np.stack(exhaustive_frame())[None]
    out = []
    for f in range(3):
        shared = inputs.syn1(h, w, 90 + f).astype(np.uint16)
        out.append(np.stack([((shared * 3 + inputs.syn1(h, w, 100 + 3 * f + c)) // 4).astype(np.uint8) for c in range(3)]))
    return np.stack(out)


def _source(frames, layout):
    """(what encode_batch_from takes, scale): the frames in device memory in one of the three layouts."""
    torch = _torch()
    if layout == "nchw uint8":
        return _dev(frames), 1.0
    if layout == "nhwc uint8":
        return _dev(frames.transpose(0, 2, 3, 1)).permute(0, 3, 1, 2), 1.0
    t = _dev((frames.astype(np.float32) / 255.0).astype(np.float16)).contiguous(memory_format=torch.channels_last)
    return t, 255.0                                             # (|f16(p / 255) * 255 - p| < 255 * 2^-11: the collected plane is the frame)


def _transformed(pkg, frames):
    """The 3 F planes whose streams color="rct" writes, n-major."""
    return [p for fr in frames for p in pkg.rct_forward(fr[0], fr[1], fr[2])]


def _streams(ctx, pkg, h, w, effort=1):
    """The frames of a geometry and their colour streams, made once."""
    key = (h, w, effort)
    if key not in _cache:
        frames = _frames(h, w)
        got = ctx.encode_batch_from(_dev(frames), effort=effort, color="rct")
        assert all(s is not None for s in got)
        _cache[key] = (frames, got)
    return _cache[key]


@pytest.mark.parametrize("effort", (0, 1, 2, 3))
@pytest.mark.parametrize("geom", GEOMS)
def test_encode_equals_the_plain_call_on_the_transformed_planes(ctx, pkg, oracle, geom, effort):
    h, w = geom
    frames = _frames(h, w)
    planes = _transformed(pkg, frames)
    want = ctx.encode_batch_from(_dev(np.stack(planes)), effort=effort)
    assert all(s is not None for s in want) and len(want) == 3 * len(frames)
    for layout in LAYOUTS if h != 256 else LAYOUTS[:1]:
        src, scale = _source(frames, layout)
        got = ctx.encode_batch_from(src, scale=scale, effort=effort, color="rct")
        assert got == want, (layout, [a == b for a, b in zip(got, want)])
        assert ctx.encode_batch_from([src[n][c] for n in range(len(frames)) for c in range(3)], scale=scale, effort=effort, color="rct") == want, layout
    for c in range(3):                                         # one frame per mode against the oracle
        assert want[c] == (oracle.qencode(planes[c]) if effort == 0 else oracle.encode(planes[c], 0, effort)[0]), c
    # the streams differ from those of the untransformed planes: the transform took place
    assert ctx.encode_batch_from(_dev(frames), effort=effort)[0] != want[0]


@pytest.mark.parametrize("effort", (0, 1))
@pytest.mark.parametrize("geom", GEOMS)
def test_indexed_encode_equals_the_plain_call_on_the_transformed_planes(ctx, pkg, geom, effort):
    h, w = geom
    frames = _frames(h, w)
    planes = _dev(np.stack(_transformed(pkg, frames)))
    for band_rows in (5, 0):
        want = ctx.encode_batch_from(planes, effort=effort, every_rows=EVERY, band_rows=band_rows)
        assert all(s is not None and x is not None for s, x in want)
        for layout in LAYOUTS if h != 256 else LAYOUTS[1:2]:
            src, scale = _source(frames, layout)
            got = ctx.encode_batch_from(src, scale=scale, effort=effort, every_rows=EVERY, band_rows=band_rows, color="rct")
            assert got == want, (layout, band_rows)


def _decode(ctx, how, pairs, out, **kw):
    if how == "indexed":
        return ctx.decode_batch_indexed_into(pairs, out, layout="any", color="rct", **kw)
    return ctx.decode_batch_into([s for s, _ in pairs], out, layout="any", color="rct", **kw)


def _kept(pkg, how):
    """The indexed call keeps no device resource; the plain one has the context's grow-only workspace."""
    return _live(pkg) if how == "indexed" else contextlib.nullcontext()


def _pairs(ctx, pkg, streams, Rs=(7, 5, 16)):
    """(stream, index) per plane: another R for every plane of a frame, packed and unpacked indexes mixed."""
    out = []
    for k, s in enumerate(streams):
        ix = ctx.build_index(s, Rs[k % 3])
        out.append((s, pkg.pack_index(ix) if k % 2 else ix))
    return out


def _norms(n_frames):
    return [CHANNEL_NORMS[c][0] for _ in range(n_frames) for c in range(3)], [CHANNEL_NORMS[c][1] for _ in range(n_frames) for c in range(3)]


@pytest.mark.parametrize("how", ("indexed", "plain"))
@pytest.mark.parametrize("geom", GEOMS)
def test_decode_gives_the_original_frames(ctx, pkg, geom, how):
    """uint8 NHWC and channels-last float16 with a mean and std per channel, whole and a window of rows and columns."""
    torch = _torch()
    h, w = geom
    frames, streams = _streams(ctx, pkg, h, w)
    F = len(frames)
    pairs = _pairs(ctx, pkg, streams)
    assert any(pkg.index_is_packed(x) for _, x in pairs) and not all(pkg.index_is_packed(x) for _, x in pairs)
    out = _filled((F, h, w, 3), 0)
    info = {}
    with _kept(pkg, how):
        assert _decode(ctx, how, pairs, out.permute(0, 3, 1, 2), info=info) == [0] * (3 * F) and info["rc"] == 0
    assert ctx.deliver_stats() == (3 * F, 3 * F)
    assert np.array_equal(_bits(out), frames.transpose(0, 2, 3, 1)), how
    # without color the same streams give the transformed planes
    plain = _filled((F, h, w, 3), 0)
    call = ctx.decode_batch_indexed_into if how == "indexed" else ctx.decode_batch_into
    assert call(pairs if how == "indexed" else streams, plain.permute(0, 3, 1, 2), layout="any") == [0] * (3 * F)
    assert np.array_equal(_bits(plain).transpose(0, 3, 1, 2).reshape(3 * F, h, w), np.stack(_transformed(pkg, frames)))
    scales, biases = _norms(F)
    f16 = _filled((F, h, w, 3), 1).permute(0, 3, 1, 2)
    assert f16.is_contiguous(memory_format=torch.channels_last)
    assert _decode(ctx, how, pairs, f16, scale=scales, bias=biases) == [0] * (3 * F)
    got = _bits(f16)
    for f in range(F):
        for c in range(3):
            assert np.array_equal(got[f, c], _elements(frames[f, c], 1, *CHANNEL_NORMS[c])), (how, f, c)
    r, c_ = (12, h - 1), (5, w - 3)                             # the rows start in another segment of every plane's index
    for fmt in (0, 1):
        win = _filled((F, r[1] - r[0], c_[1] - c_[0], 3), fmt).permute(0, 3, 1, 2)
        norm = dict(scale=scales, bias=biases) if fmt else {}
        assert _decode(ctx, how, pairs, win, rows=r, cols=c_, **norm) == [0] * (3 * F)
        got = _bits(win)
        for f in range(F):
            for c in range(3):
                want = _elements(frames[f, c, r[0]:r[1], c_[0]:c_[1]], fmt, *(CHANNEL_NORMS[c] if fmt else (1.0, 0.0)))
                assert np.array_equal(got[f, c], want), (how, fmt, f, c)
    # planar destinations: a list of three [h, w] tensors per frame
    flat = _filled((3 * F, h, w), 0)
    assert _decode(ctx, how, pairs, [flat[k] for k in range(3 * F)]) == [0] * (3 * F)
    assert np.array_equal(_bits(flat).reshape(F, 3, h, w), frames)


@pytest.mark.parametrize("how", ("indexed", "plain"))
def test_planes_of_different_classes_in_one_frame(ctx, pkg, oracle, how):
    """G is an -e1 stream and the differences are QNBLIC (frame 0), or -e2 and -e3 (frame 1): the three planes of a frame
    fall into different (codec, effort) classes -- in the plain call: different chunks on different streams."""
    h, w = GEOMS[0]
    frames = _frames(h, w)[:2]
    planes = _transformed(pkg, frames)
    enc = lambda p, e: oracle.qencode(p) if e == 0 else oracle.encode(p, 0, e)[0]
    streams = [enc(p, e) for p, e in zip(planes, (0, 1, 0, 2, 1, 3))]
    pairs = _pairs(ctx, pkg, streams)
    scales, biases = _norms(2)
    for fmt in (0, 1):
        out = _filled((2, h, w, 3), fmt)
        norm = dict(scale=scales, bias=biases) if fmt else {}
        info = {}
        with _kept(pkg, how):
            assert _decode(ctx, how, pairs, out.permute(0, 3, 1, 2), info=info, **norm) == [0] * 6 and info["rc"] == 0
        got = _bits(out)
        for f in range(2):
            for c in range(3):
                assert np.array_equal(got[f, :, :, c], _elements(frames[f, c], fmt, *(CHANNEL_NORMS[c] if fmt else (1.0, 0.0)))), (how, fmt, f, c)


def test_encode_refusals_cost_their_frame_only(ctx, pkg):
    torch = _torch()
    h, w = GEOMS[0]
    frames = _frames(h, w)
    want = _streams(ctx, pkg, h, w)[1]
    src = _dev(frames.transpose(0, 2, 3, 1))
    views = lambda: [src[n, :, :, c] for n in range(3) for c in range(3)]
    for what in ("unequal sizes", "a host pointer"):
        v = views()
        if what == "unequal sizes":
            v[5] = src[1, :h - 1, :, 2]
        else:
            v[4] = torch.from_numpy(np.ascontiguousarray(frames[1, 1]))
        for kw in ({}, dict(effort=0), dict(every_rows=EVERY), dict(effort=0, every_rows=EVERY)):
            info = {}
            got = ctx.encode_batch_from(v, info=info, color="rct", **kw)
            if "every_rows" in kw:
                assert got[3:6] == [(None, None)] * 3 and all(s is not None and x is not None for s, x in got[:3] + got[6:]), (what, kw)
                got = [s for s, _ in got]
            assert got[3:6] == [None] * 3, (what, kw)
            if kw in ({}, dict(every_rows=EVERY)):
                assert got[:3] == want[:3] and got[6:] == want[6:], (what, kw)
            else:
                assert got[:3] == _streams(ctx, pkg, h, w, 0)[1][:3] and got[6:] == _streams(ctx, pkg, h, w, 0)[1][6:], (what, kw)
    # near-lossless, and a batch that is no whole number of frames: the whole call
    with pytest.raises(ValueError):
        ctx.encode_batch_from(views(), near=2, color="rct")
    with pytest.raises(ValueError):
        ctx.encode_batch_from(views(), near=[0] * 8 + [2], effort=[1] * 8 + [2], color="rct")
    with pytest.raises(ValueError):
        ctx.encode_batch_from(views()[:8], color="rct")
    with pytest.raises(ValueError):
        ctx.encode_batch_from(src, color="rct")                # [N, H, W, 3] as it is: four channels of width 3
    with pytest.raises(ValueError):
        ctx.encode_batch_from(views(), color="ycocg")
    with pytest.raises(ValueError):
        ctx.encode_batch_from(views(), color="rct", recon_out=_filled((9, h, w), 0))
    srcs, fmt = pkg._srcs_of(views()[:8], None, None)          # the C calls themselves: n % 3, and the call that has no colour frames
    for kw in ({}, dict(effort=0), dict(every_rows=EVERY)):
        with pytest.raises(ValueError):
            ctx.encode_from_srcs(srcs, fmt | pkg.FORMAT_RCT, **kw)
    srcs, fmt = pkg._srcs_of(views(), None, None)
    rec = _filled((9, h, w), 0)
    dests = [(rec[k].data_ptr(), w, 1, h * w, 0, 0, 0, 0, 1.0, 0.0) for k in range(9)]
    with pytest.raises(ValueError):
        ctx.encode_from_srcs(srcs, fmt | pkg.FORMAT_RCT, recon_dests=dests, recon_fmt=0)
    assert bool((rec == PATTERN).all())
    assert ctx.encode_from_srcs(srcs, fmt | pkg.FORMAT_RCT) == want


@pytest.mark.parametrize("how", ("indexed", "plain"))
def test_decode_refusals_and_failures_cost_their_frame_only(ctx, pkg, how):
    torch = _torch()
    h, w = GEOMS[0]
    frames, streams = _streams(ctx, pkg, h, w)
    pairs = _pairs(ctx, pkg, streams, Rs=(7, 7, 7))
    norm = CHANNEL_NORMS[0]
    fill = int.from_bytes(bytes([PATTERN]) * 2, "little")

    def check(out, status, info, frame1):
        assert status == [0, 0, 0, -1, -1, -1, 0, 0, 0] and info["rc"] == -1
        got = _bits(out)
        for f in (0, 2):
            for c in range(3):
                assert np.array_equal(got[f, :, :, c], _elements(frames[f, c], 1, *norm)), (f, c)
        assert (got[1] == frame1).all()

    # destinations with unequal windows: the frame is refused and not written
    out = _filled((3, h, w, 3), 1)
    views = [out[n, :, :, c] for n in range(3) for c in range(3)]
    views[3] = out[1, 1:, :, 0]
    rows = [(0, h)] * 9
    rows[3] = (1, h)
    info = {}
    with _kept(pkg, how):
        status = _decode(ctx, how, pairs, views, rows=rows, scale=norm[0], bias=norm[1], info=info)
    check(out, status, info, fill)
    # a refused destination (a host tensor) among three
    out = _filled((3, h, w, 3), 1)
    views = [out[n, :, :, c] for n in range(3) for c in range(3)]
    cpu = torch.from_numpy(np.full((h, w, 2), PATTERN, np.uint8)).view(torch.float16)[:, :, 0]
    views[4] = cpu
    info = {}
    status = _decode(ctx, how, pairs, views, scale=norm[0], bias=norm[1], info=info)
    check(out, status, info, fill)
    assert bool((cpu.view(torch.uint8) == PATTERN).all())
    # a plane that fails on the device: zeros in all three windows, three statuses -1
    broken = list(pairs)
    if how == "plain":
        s = streams[5]
        broken[5] = (s[:len(s) * 2 // 3], pairs[5][1])
        assert ctx.decode_batch([broken[5][0]])[0] is None
    else:
        forged = _forge(ctx.build_index(streams[4], 7), 4, "n", 1, w, "row1")
        assert pkg.check_index(forged, streams[4])
        broken[4] = (streams[4], forged)
    out = _filled((3, h, w, 3), 1)
    info = {}
    with _kept(pkg, how):
        status = _decode(ctx, how, broken, out.permute(0, 3, 1, 2), scale=norm[0], bias=norm[1], info=info)
    check(out, status, info, 0)
    # no whole number of frames, and a channel count that is not 3
    with pytest.raises(ValueError):
        _decode(ctx, how, pairs[:8], [out[0, :, :, 0]] * 8)
    with pytest.raises(ValueError):
        _decode(ctx, how, pairs, _filled((9, h, w), 1))
    dests = [(out[k // 3, :, :, k % 3].data_ptr(), w * 6, 6, out.numel() * 2, 0, 0, 0, 0, 1.0, 0.0) for k in range(8)]
    before = _bits(out).copy()
    call = (lambda: ctx.decode_batch_indexed_to_ex(pairs[:8], dests, 1 | pkg.FORMAT_RCT)) if how == "indexed" else \
           (lambda: ctx.decode_batch_to_ex(streams[:8], dests, 1 | pkg.FORMAT_RCT))
    assert call() == [-1] * 8 and np.array_equal(_bits(out), before)


def test_calls_without_color_return_what_they_returned(ctx, pkg):
    """The same inputs without the flag: the streams of the untransformed planes, as encode_batch / qencode_batch /
    encode_batch_indexed make them of the host planes, and decode_batch's planes."""
    h, w = GEOMS[1]
    frames = _frames(h, w)
    planes = [np.ascontiguousarray(frames[f, c]) for f in range(len(frames)) for c in range(3)]
    src, scale = _source(frames, "nhwc uint8")
    got = ctx.encode_batch_from(src)
    assert got == ctx.encode_batch(planes)
    assert ctx.encode_batch_from(src, effort=0) == ctx.qencode_batch(planes)
    assert ctx.encode_batch_from(src, every_rows=EVERY) == ctx.encode_batch_indexed(planes, EVERY)
    assert ctx.encode_batch_from(src, effort=0, every_rows=EVERY) == ctx.qencode_batch_indexed(planes, EVERY)
    out = _filled((len(frames), h, w, 3), 0)
    assert ctx.decode_batch_into(got, out.permute(0, 3, 1, 2), layout="any") == [0] * len(planes)
    host = [p[0] for p in ctx.decode_batch(got)]
    assert np.array_equal(_bits(out).transpose(0, 3, 1, 2).reshape(len(planes), h, w), np.stack(host)) and all(np.array_equal(a, b) for a, b in zip(host, planes))
    pairs = [(s, ctx.build_index(s, 5)) for s in got]
    out = _filled((len(frames), h, w, 3), 0)
    assert ctx.decode_batch_indexed_into(pairs, out.permute(0, 3, 1, 2), layout="any") == [0] * len(planes)
    assert np.array_equal(_bits(out).transpose(0, 3, 1, 2).reshape(len(planes), h, w), np.stack(planes))
