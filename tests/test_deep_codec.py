"""GPU suite (-m gpu): deep pixels through the public calls.  The streams and indexes of ``encode_batch_from(..., deep=...)``
from uint16 and int16 tensors, contiguous and a strided view, at efforts 0 .. 3 and through both indexed calls, are byte for
byte those of the same call on ``deep_forward``'s planes, a sample of them the oracle's; ``decode_batch_into`` /
``decode_batch_indexed_into`` with the modes return the source exactly into uint16 / int16, and numpy's expression bit for bit
into a channels-last float16 tensor with scale and bias; a row range with an index and a column window; near = 3 on the low
plane; a low stream cut short; what is refused; and ``deep_plan`` on the constructed classes."""
import numpy as np
import pytest

import deep_inputs as di
from test_rct_codec import _dev, _torch

pytestmark = pytest.mark.gpu

GEOMS = ((96, 80), (33, 17))
N = 3                                                          # deep images per call
EVERY = 16
MIXED = (1, 0, 1)                                              # bit 0 per image
PATTERN = 0x5A


@pytest.fixture(scope="module")
def ctx(pkg, gpu_ctx):
    """A context of this module's own (made after the session's, which initialises torch first)."""
    c = pkg.Context(device=0, n_slots=3, n_coders=3)
    yield c
    c.close()


_cache = {}


def _images(h, w, signed):
    """[N, h, w] uint16 or int16: ramps with noise that cross many high-byte steps, the edge values among them."""
    key = (h, w, signed)
    if key not in _cache:
        rng = np.random.default_rng(300 + h + (7 if signed else 0))
        _cache[key] = np.stack([di.random_image(rng, h, w, signed) for _ in range(N)])
    return _cache[key]


def _modes(deep, signed):
    bits = {"plain": (0,) * N, "fold": (1,) * N}.get(deep, deep) if isinstance(deep, str) else deep
    return np.array([b | (2 if signed else 0) for b in bits], np.uint8)


def _planes(pkg, x, modes):
    """The 2 N planes whose streams deep=modes writes: high, low, high, low, ..."""
    return [p for k in range(len(x)) for p in pkg.deep_forward(x[k], int(modes[k]))]


def _strided(x):
    """The images as a view with a step of 4 bytes and a pitch of its own: every second element of a wider tensor of junk."""
    wide = np.full(x.shape[:2] + (x.shape[2] + 3, 2), 0x7B7B, x.dtype)
    wide[:, :, :x.shape[2], 0] = x
    return _dev(wide)[:, :, :x.shape[2], 0]


def _filled(shape, dtype):
    """A device tensor of this shape and dtype whose every byte is the pattern."""
    t = _torch()
    return t.full(tuple(shape[:-1]) + (shape[-1] * np.dtype(dtype).itemsize,), PATTERN, dtype=t.uint8, device="cuda").view(getattr(t, np.dtype(dtype).name))


def _host(tensor, dtype):
    return tensor.contiguous().view(_torch().uint8).cpu().numpy().view(dtype)


def _pairs(ctx, pkg, streams, Rs=(7, 5, 16)):
    out = []
    for k, s in enumerate(streams):
        ix = ctx.build_index(s, Rs[k % 3])
        out.append((s, pkg.pack_index(ix) if k % 2 else ix))
    return out


def _decode(ctx, how, pairs, out, deep, **kw):
    if how == "indexed":
        return ctx.decode_batch_indexed_into(pairs, out, deep=deep, **kw)
    return ctx.decode_batch_into([s for s, _ in pairs], out, deep=deep, **kw)


@pytest.mark.parametrize("signed", (False, True), ids=("uint16", "int16"))
@pytest.mark.parametrize("effort", (0, 1, 2, 3))
def test_streams_and_indexes_are_those_of_the_planes(ctx, pkg, oracle, effort, signed):
    for h, w in GEOMS:
        x = _images(h, w, signed)
        for deep in ("plain", "fold", MIXED) if effort < 2 else ("fold", MIXED):
            modes = _modes(deep, signed)
            planes = _planes(pkg, x, modes)
            dev_planes = _dev(np.stack(planes))
            want = ctx.encode_batch_from(dev_planes, effort=effort)
            assert len(want) == 2 * N and all(s is not None for s in want)
            arg = deep if isinstance(deep, str) else modes
            before = ctx.deep_plan_stats()
            assert ctx.encode_batch_from(_dev(x), effort=effort, deep=arg) == want, (h, w, deep)
            assert ctx.deep_plan_stats()["collect_launches"] == before["collect_launches"] + 1       # ONE launch collects every plane of the call
            assert ctx.encode_batch_from(_strided(x), effort=effort, deep=arg) == want, (h, w, deep, "strided")
            assert ctx.encode_batch_from([_dev(x)[k] for k in range(N)], effort=effort, deep=modes) == want
            if effort < 2:                                     # both indexed calls
                want_x = ctx.encode_batch_from(dev_planes, effort=effort, every_rows=EVERY, band_rows=5)
                assert all(s is not None and i is not None for s, i in want_x)
                assert ctx.encode_batch_from(_strided(x), effort=effort, every_rows=EVERY, band_rows=5, deep=arg) == want_x, (h, w, deep)
            for k in (0, 1, 2 * N - 1):                        # a high plane, a low plane, the call's last low plane against the oracle
                assert want[k] == (oracle.qencode(planes[k]) if effort == 0 else oracle.encode(planes[k], 0, effort)[0]), k


@pytest.mark.parametrize("signed", (False, True), ids=("uint16", "int16"))
@pytest.mark.parametrize("how", ("plain", "indexed"))
def test_decode_returns_the_source(ctx, pkg, how, signed):
    dtype = np.int16 if signed else np.uint16
    for h, w in GEOMS:
        x = _images(h, w, signed)
        for deep in ("fold", MIXED):
            modes = _modes(deep, signed)
            streams = ctx.encode_batch_from(_dev(x), deep=modes, effort=0 if deep == "fold" else 1)
            pairs = _pairs(ctx, pkg, streams)
            out = _filled((N, h, w), dtype)
            before = ctx.deep_plan_stats()
            assert _decode(ctx, how, pairs, out, deep if isinstance(deep, str) else modes) == [0] * (2 * N)
            assert ctx.deep_plan_stats()["deliver_launches"] == before["deliver_launches"] + 1
            assert np.array_equal(_host(out, dtype), x), (h, w, deep)
            # a strided destination with a pitch of its own: the bytes between the elements keep their contents
            wide = _filled((N, h, w + 2, 3), dtype)
            assert _decode(ctx, how, pairs, wide[:, :, 1:w + 1, 1], modes) == [0] * (2 * N)
            got = _host(wide, dtype)
            assert np.array_equal(got[:, :, 1:w + 1, 1], x)
            got[:, :, 1:w + 1, 1] = dtype(0x5A5A)
            assert (got.view(np.uint8) == PATTERN).all()


@pytest.mark.parametrize("how", ("plain", "indexed"))
def test_float16_channels_last_with_scale_and_bias(ctx, pkg, how):
    h, w = GEOMS[0]
    for signed, scale, bias in ((False, 1.0 / 16.0, -100.0), (True, 1.0 / 1000.0, 1.024), (False, 1.0, 0.0)):
        x = _images(h, w, signed)
        modes = _modes(MIXED, signed)
        pairs = _pairs(ctx, pkg, ctx.encode_batch_from(_dev(x), deep=modes))
        out = _filled((N, h, w, 2), np.float16)                 # [N, H, W, C]: the images go to channel 1
        scales = [scale, scale * 2, scale]
        assert _decode(ctx, how, pairs, [out[k, :, :, 1] for k in range(N)], modes, scale=scales, bias=bias) == [0] * (2 * N)
        got = _host(out, np.uint16)
        for k in range(N):
            with np.errstate(over="ignore"):
                want = (x[k].astype(np.float32) * np.float32(scales[k]) + np.float32(bias)).astype(np.float16)
            assert np.array_equal(got[k, :, :, 1], want.view(np.uint16)), (signed, k)      # (scale 1: the values above 65504 are infinities)
        assert (got[:, :, :, 0] == 0x5A5A).all()
    if how == "plain":
        assert np.isinf(want).any()


def test_a_row_range_with_an_index_and_a_column_window(ctx, pkg):
    h, w = GEOMS[0]
    x = _images(h, w, True)
    modes = _modes(MIXED, True)
    pairs = _pairs(ctx, pkg, ctx.encode_batch_from(_dev(x), deep=modes))
    rows, cols = [(37, 61), (0, 0), (90, 96)], [(3, 70), (11, 12), (0, 0)]
    shapes = [(24, 67), (h, 1), (6, w)]
    for how in ("indexed", "plain"):
        outs = [_filled(s, np.float32) for s in shapes]
        info = {}
        assert _decode(ctx, how, pairs, outs, modes, rows=rows, cols=cols, scale=0.5, bias=0.25, info=info) == [0] * (2 * N) and info["rc"] == 0
        for k, o in enumerate(outs):
            (r0, r1), (c0, c1) = rows[k], cols[k]
            want = x[k, r0:r1 or h, c0:c1 or w].astype(np.float32) * np.float32(0.5) + np.float32(0.25)
            assert np.array_equal(_host(o, np.float32), want), (how, k)
    # the pairs of the indexed encoder decode alike
    enc = ctx.encode_batch_from(_dev(x), deep=modes, every_rows=EVERY)
    out = _filled((N, 24, 67), np.int16)
    assert ctx.decode_batch_indexed_into(enc, out, deep=modes, rows=(37, 61), cols=(3, 70)) == [0] * (2 * N)
    assert np.array_equal(_host(out, np.int16), x[:, 37:61, 3:70])


@pytest.mark.parametrize("signed", (False, True), ids=("uint16", "int16"))
def test_near_on_the_low_plane_bounds_the_error(ctx, pkg, signed):
    """near = 3 on the low plane, the high plane lossless: the low plane's reconstruction stays in 0 .. 255, the high byte is
    exact and the fold keeps distances, so max |x' - x| <= 3, folded or not -- on images that cross many high-byte steps."""
    dtype = np.int16 if signed else np.uint16
    h, w = GEOMS[0]
    x = _images(h, w, signed)
    assert len(np.unique(di.unsigned_of(x) // 256)) > 8
    for deep in ("plain", "fold"):
        info = {}
        streams = ctx.encode_batch_from(_dev(x), deep=deep, near=3, effort=2, info=info)
        lossless = ctx.encode_batch_from(_dev(x), deep=deep, effort=2)
        assert all(s is not None for s in streams) and streams[0::2] == lossless[0::2] and all(len(a) < len(b) for a, b in zip(streams[1::2], lossless[1::2]))
        out = _filled((N, h, w), dtype)
        assert ctx.decode_batch_into(streams, out, deep=deep) == [0] * (2 * N)
        err = np.abs(_host(out, dtype).astype(np.int64) - x.astype(np.int64))
        print(deep, "max |x' - x| =", int(err.max()))
        assert 0 < int(err.max()) <= 3
        modes = _modes(deep, signed)
        for k in range(N):                                     # the host reconstructions are the two planes'
            assert np.array_equal(pkg.deep_inverse(info["recons"][2 * k], info["recons"][2 * k + 1], int(modes[k])), _host(out, dtype)[k])
    with pytest.raises(ValueError):                            # the high plane must be lossless
        ctx.encode_batch_from(_dev(x), deep="fold", near=[1, 0] + [0] * (2 * N - 2), effort=2)


@pytest.mark.parametrize("how", ("plain", "indexed"))
def test_a_low_stream_cut_short(ctx, pkg, how):
    """-1 for both streams of the image and zeros in its window; the neighbouring images are intact."""
    from test_indexed_batch_decode import _forge
    h, w = GEOMS[0]
    x = _images(h, w, False)
    modes = _modes(MIXED, False)
    streams = ctx.encode_batch_from(_dev(x), deep=modes)
    pairs = _pairs(ctx, pkg, streams, Rs=(7, 7, 7))
    for k in (3, 2):                                           # image 1's low plane, then its high plane
        bad = list(pairs)
        if how == "plain":
            bad[k] = (streams[k][:len(streams[k]) * 2 // 3], pairs[k][1])
            assert ctx.decode_batch([bad[k][0]])[0] is None
        else:
            forged = _forge(ctx.build_index(streams[k], 7), 4, "n", 1, w, "row1")
            assert pkg.check_index(forged, streams[k])
            bad[k] = (streams[k], forged)
        out = _filled((N, h, w), np.uint16)
        info = {}
        assert _decode(ctx, how, bad, out, modes, info=info) == [0, 0, -1, -1, 0, 0] and info["rc"] == -1, (how, k)
        got = _host(out, np.uint16)
        assert np.array_equal(got[0], x[0]) and np.array_equal(got[2], x[2]) and (got[1] == 0).all()


def test_refusals(ctx, pkg):
    h, w = GEOMS[0]
    x = _images(h, w, False)
    s = _images(h, w, True)
    src = _dev(x)
    modes = _modes(MIXED, False)
    streams = ctx.encode_batch_from(src, deep=modes)
    pairs = _pairs(ctx, pkg, streams)
    # the whole call: an invalid byte, bit 1 against the dtype, a high plane with a near -- ValueError, nothing launched
    before = ctx.deep_plan_stats()
    for bad in ([0, 4, 1], [0, 0xFF, 0], [2, 2, 2], [0, 1]):
        for kw in ({}, dict(effort=0), dict(every_rows=EVERY), dict(effort=0, every_rows=EVERY)):
            with pytest.raises(ValueError):
                ctx.encode_batch_from(src, deep=bad, **kw)
    with pytest.raises(ValueError):
        ctx.encode_batch_from(_dev(s), deep=[0, 0, 0])
    for bad in (dict(color="rct"), dict(stack="delta", depth=1), dict(recon_out=_filled((N, h, w), np.uint8))):
        with pytest.raises(ValueError):
            ctx.encode_batch_from(src, deep="fold", **bad)
    with pytest.raises(ValueError):
        ctx.encode_batch_from(_dev(x.astype(np.float32)), deep="fold")
    with pytest.raises(ValueError):
        ctx.encode_batch_from(src, deep="folded")
    assert ctx.deep_plan_stats() == before
    for how in ("plain", "indexed"):
        for bad in ([0, 4, 1], [0, 0xFF, 0]):
            out = _filled((N, h, w), np.uint16)
            info = {}
            assert _decode(ctx, how, pairs, out, bad, info=info) == [-1] * (2 * N) and info["rc"] == -1
            assert (_host(out, np.uint8) == PATTERN).all()
        with pytest.raises(ValueError):
            _decode(ctx, how, pairs, _filled((N, h, w), np.uint16), modes, color="rct")
        with pytest.raises(ValueError):
            _decode(ctx, how, pairs, _filled((N, h, w), np.uint8), modes)
    # the existing calls keep refusing 16-bit sources and destinations
    with pytest.raises(ValueError):
        ctx.encode_batch_from(src)
    with pytest.raises(ValueError):
        ctx.decode_batch_into(streams[:N], _filled((N, h, w), np.uint16))
    # that image alone: a signedness that contradicts the mode, unequal sizes, a stream that does not parse, a destination
    # that is not its window's shape -- both statuses -1, nothing written, the neighbours delivered
    other = ctx.encode_batch_from(_dev(x[:1, :h - 1]), deep="plain")
    for how in ("plain", "indexed"):
        for case in ("sign", "size", "garbage", "dest"):
            p, m, dtype = list(pairs), modes.copy(), np.uint16
            outs = [_filled((h, w), np.uint16) for _ in range(N)]
            if case == "sign":
                m[1] |= 2                                      # a signed image into a uint16 tensor
            elif case == "size":
                p[3] = (other[1], ctx.build_index(other[1], 7))
            elif case == "garbage":
                p[2] = (b"not a stream", pairs[2][1])
            else:
                outs[1] = _filled((h, w - 1), np.uint16)
            info = {}
            assert _decode(ctx, how, p, outs, m, info=info) == [0, 0, -1, -1, 0, 0] and info["rc"] == -1, (how, case)
            assert (_host(outs[1], np.uint8) == PATTERN).all(), (how, case)
            assert np.array_equal(_host(outs[0], dtype), x[0]) and np.array_equal(_host(outs[2], dtype), x[2]), (how, case)
    # the encoder: a source of a size the encoder does not take is refused alone
    views = [src[k] for k in range(N)]
    views[1] = src[1][:, :0]
    got = ctx.encode_batch_from(views, deep=modes)
    assert got[2:4] == [None, None] and got[:2] == streams[:2] and got[4:] == streams[4:]


def test_the_plan_on_the_classes(ctx, pkg):
    """ONE k_deep_cost launch over the classes: the costs and the range are the host walk's, the mode is the rule's, and it is
    the mode whose two streams are smaller at -e1 (ties plan as plain).  Signed sources plan alike, with bit 1 set."""
    names = list(di.CLASSES)
    x = np.stack([di.class_image(n) for n in names])
    before = ctx.deep_plan_stats()
    modes, costs, ranges = ctx.deep_plan(_dev(x), costs=True)
    after = ctx.deep_plan_stats()
    assert after["plan_launches"] == before["plan_launches"] + 1 and after["images"] == before["images"] + len(names) and after["plan_ms"] > 0
    for k, name in enumerate(names):
        sums = pkg.deep_cost_host(x[k], 0)
        assert np.array_equal(costs[k], sums[:3]) and tuple(ranges[k]) == (int(x[k].min()), int(x[k].max())), name
        assert modes[k] == pkg.deep_choose(costs[k], 0) == di.CLASSES[name], name
    info = {}
    planned = ctx.encode_batch_from(_dev(x), deep="plan", info=info)
    assert np.array_equal(info["deep_modes"], modes)
    size = {d: ctx.encode_batch_from(_dev(x), deep=d) for d in ("plain", "fold")}
    for k, name in enumerate(names):
        plain, fold = (sum(len(s) for s in size[d][2 * k:2 * k + 2]) for d in ("plain", "fold"))
        assert planned[2 * k:2 * k + 2] == size["fold" if modes[k] & 1 else "plain"][2 * k:2 * k + 2]
        print(name, "plain", plain, "fold", fold, "planned", "fold" if modes[k] & 1 else "plain")
        if name in di.TIES:
            assert plain == fold and modes[k] == 0, name
        else:
            assert (modes[k] & 1) == (1 if fold < plain else 0), name
    xs = (x ^ np.uint16(0x8000)).view(np.int16)
    smodes, scosts, sranges = ctx.deep_plan(_strided(xs), costs=True)
    assert np.array_equal(smodes, modes | 2) and np.array_equal(scosts, costs) and np.array_equal(sranges, ranges.astype(np.int64) - 32768)
    # a refused source: 0xFF and zeros for it alone, and "plan" encodes the others
    views = [_dev(x)[k] for k in range(3)]
    views[1] = views[1][:, :0]
    m, c, r = ctx.deep_plan(views, costs=True)
    assert list(m) == [modes[0], 0xFF, modes[2]] and not c[1].any() and not r[1].any()
    got = ctx.encode_batch_from(views, deep="plan")
    assert got[2:4] == [None, None] and got[:2] == planned[:2] and got[4:6] == planned[4:6]
