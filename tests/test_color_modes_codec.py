"""GPU suite (-m gpu): per-frame colour modes through the public calls.  For each of the ten modes, and for a call with
another mode in every frame, the streams of ``encode_batch_from(..., color=modes)`` at -e1, at effort 0 and through both
indexed calls are byte for byte those of the same call without ``color`` on the host-transformed planes
(``rct_forward(mode)``), and ``decode_batch_into`` / ``decode_batch_indexed_into`` with the modes return the original
frames into uint8 NHWC and channels-last float16 with a scale and bias per channel, whole and as a window; every mode
0x0D is ``color="rct"``; a frame of mode 0 stands beside a damaged frame; what is refused; and ``color_plan`` on the four
constructed classes gives the modes of the host test, with which the frames round-trip."""
import numpy as np
import pytest

import color_plan_inputs as ci
from rct_inputs import CHANNEL_NORMS
from test_decode_to_device import _bits, _elements, _filled
from test_deliver_strided_host import PATTERN
from test_indexed_batch_decode import _forge
from test_rct_codec import _dev, _norms, _pairs, _source, _torch

pytestmark = pytest.mark.gpu

GEOMS = ((48, 80), (33, 130))
EVERY = 16
MIXED = (0x08, 0x00, 0x0D, 0x06)                                # another mode in every frame, a plain one among them
MODE_SETS = tuple((m,) * 4 for m in (0, 4, 8, 12, 5, 9, 13, 6, 10, 14)) + (MIXED,)

_cache = {}


@pytest.fixture(scope="module")
def ctx(pkg, gpu_ctx):
    """A context of this module's own (made after the session's, which initialises torch first)."""
    c = pkg.Context(device=0, n_slots=3, n_coders=3)
    yield c
    c.close()


def _frames(h, w):
    """[4, 3, h, w] uint8: the four classes of color_plan_inputs."""
    if (h, w) not in _cache:
        _cache[(h, w)] = ci.class_frames(h, w)
    return _cache[(h, w)]


def _transformed(pkg, frames, modes):
    """The 3 F planes whose streams color=modes writes, n-major."""
    return [p for fr, m in zip(frames, modes) for p in pkg.rct_forward(fr[0], fr[1], fr[2], mode=m)]


def _decode(ctx, how, pairs, out, modes, **kw):
    if how == "indexed":
        return ctx.decode_batch_indexed_into(pairs, out, layout="any", color=modes, **kw)
    return ctx.decode_batch_into([s for s, _ in pairs], out, layout="any", color=modes, **kw)


@pytest.mark.parametrize("modes", MODE_SETS, ids=lambda m: "-".join("%02x" % v for v in sorted(set(m))) if len(set(m)) == 1 else "mixed")
@pytest.mark.parametrize("geom", GEOMS)
def test_streams_are_those_of_the_transformed_planes_and_decode_to_the_frames(ctx, pkg, geom, modes):
    h, w = geom
    frames = _frames(h, w)
    F = len(frames)
    planes = _dev(np.stack(_transformed(pkg, frames, modes)))
    nhwc, _ = _source(frames, "nhwc uint8")
    f16, f16_scale = _source(frames, "channels-last float16")
    for effort in (1, 0):
        want = ctx.encode_batch_from(planes, effort=effort)
        assert all(s is not None for s in want) and len(want) == 3 * F
        assert ctx.encode_batch_from(nhwc, effort=effort, color=modes) == want, effort
        assert ctx.encode_batch_from(f16, scale=f16_scale, effort=effort, color=np.array(modes, np.uint8)) == want, effort
        want_x = ctx.encode_batch_from(planes, effort=effort, every_rows=EVERY, band_rows=5)
        assert all(s is not None and x is not None for s, x in want_x)
        assert ctx.encode_batch_from(nhwc, effort=effort, every_rows=EVERY, band_rows=5, color=modes) == want_x, effort
        if effort == 1:
            streams = want
    if any(modes):                                             # the transform took place
        assert streams != ctx.encode_batch_from(_dev(frames))
    pairs = _pairs(ctx, pkg, streams)
    scales, biases = _norms(F)
    r, c_ = (12, h - 1), (5, w - 3)
    for how in ("plain", "indexed"):
        out = _filled((F, h, w, 3), 0)
        info = {}
        assert _decode(ctx, how, pairs, out.permute(0, 3, 1, 2), modes, info=info) == [0] * (3 * F) and info["rc"] == 0
        assert np.array_equal(_bits(out), frames.transpose(0, 2, 3, 1)), how
        half = _filled((F, h, w, 3), 1).permute(0, 3, 1, 2)
        assert half.is_contiguous(memory_format=_torch().channels_last)
        assert _decode(ctx, how, pairs, half, modes, scale=scales, bias=biases) == [0] * (3 * F)
        got = _bits(half)
        for f in range(F):
            for c in range(3):
                assert np.array_equal(got[f, c], _elements(frames[f, c], 1, *CHANNEL_NORMS[c])), (how, f, c)
        win = _filled((F, r[1] - r[0], c_[1] - c_[0], 3), 1).permute(0, 3, 1, 2)
        assert _decode(ctx, how, pairs, win, modes, rows=r, cols=c_, scale=scales, bias=biases) == [0] * (3 * F)
        got = _bits(win)
        for f in range(F):
            for c in range(3):
                assert np.array_equal(got[f, c], _elements(frames[f, c, r[0]:r[1], c_[0]:c_[1]], 1, *CHANNEL_NORMS[c])), (how, f, c)


def test_every_mode_rct_is_the_flag(ctx, pkg):
    h, w = GEOMS[0]
    frames = _frames(h, w)
    src, _ = _source(frames, "nhwc uint8")
    rct = [pkg.COLOR_RCT] * len(frames)
    for kw in ({}, dict(effort=0), dict(every_rows=EVERY), dict(effort=0, every_rows=EVERY)):
        assert ctx.encode_batch_from(src, color=rct, **kw) == ctx.encode_batch_from(src, color="rct", **kw), kw
    streams = ctx.encode_batch_from(src, color="rct")
    pairs = _pairs(ctx, pkg, streams)
    for how in ("plain", "indexed"):
        a, b = _filled((len(frames), h, w, 3), 0), _filled((len(frames), h, w, 3), 0)
        assert _decode(ctx, how, pairs, a.permute(0, 3, 1, 2), rct) == _decode(ctx, how, pairs, b.permute(0, 3, 1, 2), "rct") == [0] * 12
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), frames.transpose(0, 2, 3, 1))


@pytest.mark.parametrize("how", ("indexed", "plain"))
def test_a_plain_frame_beside_a_damaged_frame(ctx, pkg, how):
    """Frame 0 has mode 0 and frame 1 a difference mode with a damaged G stream: frame 0 is delivered, frame 1 gets zeros in
    all three windows.  A damaged G in the frame of mode 0 costs that plane alone."""
    h, w = GEOMS[0]
    frames = _frames(h, w)[:3]
    modes = (0, 0x0D, 0x08)
    streams = ctx.encode_batch_from(_dev(frames), color=modes)
    pairs = _pairs(ctx, pkg, streams, Rs=(7, 7, 7))

    def damaged(k):
        out = list(pairs)
        if how == "plain":
            out[k] = (streams[k][:len(streams[k]) * 2 // 3], pairs[k][1])
            assert ctx.decode_batch([out[k][0]])[0] is None
        else:
            forged = _forge(ctx.build_index(streams[k], 7), 4, "n", 1, w, "row1")
            assert pkg.check_index(forged, streams[k])
            out[k] = (streams[k], forged)
        return out

    for k, want_status in ((4, [0, 0, 0, -1, -1, -1, 0, 0, 0]), (1, [0, -1, 0, 0, 0, 0, 0, 0, 0])):
        out = _filled((3, h, w, 3), 0)
        info = {}
        assert _decode(ctx, how, damaged(k), out.permute(0, 3, 1, 2), modes, info=info) == want_status and info["rc"] == -1
        got = _bits(out)
        for n in range(9):
            f, c = divmod(n, 3)
            assert np.array_equal(got[f, :, :, c], frames[f, c] if want_status[n] == 0 else np.zeros((h, w), np.uint8)), (how, k, n)


def test_refusals_of_the_whole_call(ctx, pkg):
    h, w = GEOMS[0]
    frames = _frames(h, w)
    src, _ = _source(frames, "nhwc uint8")
    good = list(MIXED)
    streams = ctx.encode_batch_from(src, color=good)
    pairs = _pairs(ctx, pkg, streams)
    for bad in ([1, 0, 0, 0], [0, 0, 0xFF, 0], [0, 3, 0, 0], [0, 0, 0, 0x10], [0, 7, 0, 0]):
        for kw in ({}, dict(effort=0), dict(every_rows=EVERY), dict(effort=0, every_rows=EVERY)):
            with pytest.raises(ValueError):
                ctx.encode_batch_from(src, color=bad, **kw)
        for how in ("plain", "indexed"):
            out = _filled((4, h, w, 3), 0)
            info = {}
            assert _decode(ctx, how, pairs, out.permute(0, 3, 1, 2), bad, info=info) == [-1] * 12 and info["rc"] == -1
            assert (_bits(out) == PATTERN).all()
    for bad in ([0, 0, 0], [0] * 5, [256, 0, 0, 0], [-1, 0, 0, 0]):        # not one byte per frame
        with pytest.raises(ValueError):
            ctx.encode_batch_from(src, color=bad)
    # near > 0 in a frame whose mode is not 0: the whole call; in a frame of mode 0 it is an image like any other
    near = [0] * 12
    near[4] = 2                                                 # frame 1 of MIXED is plain
    got = ctx.encode_batch_from(src, near=near, color=good)
    assert all(s is not None for s in got) and got[:4] == streams[:4] and got[5:] == streams[5:] and got[4] != streams[4]
    near[0] = 1                                                 # frame 0 has a difference
    with pytest.raises(ValueError):
        ctx.encode_batch_from(src, near=near, color=good)
    # the C calls themselves: no whole number of frames, and the flag in a _color call
    srcs, fmt = pkg._srcs_of([src[n][c] for n in range(4) for c in range(3)], None, None)
    for kw in ({}, dict(effort=0), dict(every_rows=EVERY)):
        with pytest.raises(ValueError):
            ctx.encode_from_srcs(srcs[:11], fmt, modes=good, **kw)
        with pytest.raises(ValueError):
            ctx.encode_from_srcs(srcs, fmt | pkg.FORMAT_RCT, modes=good, **kw)
    assert ctx.encode_from_srcs(srcs, fmt, modes=good) == streams


def test_plan_then_encode_round_trips(ctx, pkg):
    h, w = GEOMS[0]
    frames = _frames(h, w)
    want = [pkg.color_choose(pkg.color_cost_numpy(*fr)) for fr in frames]
    for layout in ("nhwc uint8", "channels-last float16"):
        src, scale = _source(frames, layout)
        modes = ctx.color_plan(src, scale=scale)
        assert modes.tolist() == want, layout
        ci.check_class_modes(pkg, modes)
        streams = ctx.encode_batch_from(src, scale=scale, color=modes)
        assert streams == ctx.encode_batch_from(_dev(np.stack(_transformed(pkg, frames, modes))))
        out = _filled((4, h, w, 3), 0)
        assert ctx.decode_batch_into(streams, out.permute(0, 3, 1, 2), layout="any", color=modes) == [0] * 12
        assert np.array_equal(_bits(out), frames.transpose(0, 2, 3, 1)), layout
    # the plan pays: no larger than plain or the fixed transform on this batch
    size = lambda color: sum(len(s) for s in ctx.encode_batch_from(_dev(frames), color=color))
    print("stream bytes: plain %d, rct %d, planned %d" % (size(None), size("rct"), size(modes)))
