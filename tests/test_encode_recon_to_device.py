"""GPU suite (-m gpu): reconstructions delivered to device memory (nblic_amd_encode_batch_modes_from_to, through
``encode_batch_from(recon_out=)``).  A channels-last float16 source in every NBLIC mode: the reconstruction that lands in a
device tensor is, byte for byte, the host ``recons`` of the _from call and what ``decode_batch`` makes of the returned
streams; the streams do not change; a normalised float32 channels-last destination holds the numpy expression; and a
destination that is refused costs its reconstruction only."""
import numpy as np
import pytest

from test_decode_to_device import _bits, _elements, _filled
from test_deliver_strided_host import PATTERN

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 33, 47)
MODES = ((0, 1), (2, 1), (0, 2), (3, 3))                       # (near, effort)
SCALE, BIAS = 255.0, 0.0

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


def _source():
    """The float16 channels-last source, and its collected planes (numpy alone), n-major."""
    if "src" not in _cache:
        torch = _torch()
        import importlib
        pkg = importlib.import_module("nblic-image-compression_amd")
        rng = np.random.default_rng(2424)
        vals = (rng.random(SHAPE, np.float32) * 1.2 - 0.1).astype(np.float16)
        vals[:, :, 8:20, 10:30] = np.float16(0.5)              # a flat patch: the modes' long runs
        src = torch.from_numpy(vals).cuda().contiguous(memory_format=torch.channels_last)
        torch.cuda.synchronize()
        planes = [pkg.collect_numpy(vals[n, c], 1, SCALE, BIAS) for n in range(SHAPE[0]) for c in range(SHAPE[1])]
        _cache["src"] = (src, planes)
    return _cache["src"]


def _modes(shift):
    m = SHAPE[0] * SHAPE[1]
    return [MODES[(k + shift) % 4][0] for k in range(m)], [MODES[(k + shift) % 4][1] for k in range(m)]


@pytest.mark.parametrize("shift", range(4))
def test_reconstructions_in_a_planar_uint8_tensor(ctx, pkg, shift):
    """Every image in one of the four modes (the modes rotate with ``shift``, so every image meets every mode)."""
    src, planes = _source()
    nears, efforts = _modes(shift)
    m = len(planes)
    info = {}
    want = ctx.encode_batch_from(src, scale=SCALE, bias=BIAS, near=nears, effort=efforts, info=info)
    assert info["rc"] == 0 and all(s is not None for s in want)
    recon = _filled(SHAPE, 0)
    info2 = {}
    got = ctx.encode_batch_from(src, scale=SCALE, bias=BIAS, near=nears, effort=efforts, info=info2, recon_out=recon)
    assert info2["rc"] == 0 and got == want                    # the streams are those of the call without recon_out
    assert ctx.deliver_stats() == (m, 0)
    dev = _bits(recon).reshape(m, SHAPE[2], SHAPE[3])
    decoded = ctx.decode_batch(got)
    for k in range(m):
        assert np.array_equal(dev[k], info["recons"][k].reshape(SHAPE[2:])), (k, nears[k], efforts[k])      # the host recons of encode_from_srcs
        assert np.array_equal(dev[k], decoded[k][0]), (k, nears[k], efforts[k])                            # what a decoder produces
        err = np.abs(dev[k].astype(np.int32) - planes[k].astype(np.int32))
        assert err.max() <= nears[k], (k, nears[k], efforts[k])


def test_normalised_float32_channels_last_with_a_scale_per_image(ctx, pkg):
    src, planes = _source()
    nears, efforts = _modes(1)
    m = len(planes)
    want = ctx.encode_batch_from(src, scale=SCALE, bias=BIAS, near=nears, effort=efforts)
    recon = _filled((SHAPE[0], SHAPE[2], SHAPE[3], SHAPE[1]), 3).permute(0, 3, 1, 2)
    scales = [1.0 / 255.0, 0.0078125, 2.0 / 255.0] * SHAPE[0]
    biases = [-0.5, -1.0, 0.25] * SHAPE[0]
    got = ctx.encode_batch_from(src, scale=SCALE, bias=BIAS, near=nears, effort=efforts, recon_out=recon, recon_scale=scales, recon_bias=biases)
    assert got == want and ctx.deliver_stats() == (m, m)
    decoded = ctx.decode_batch(got)
    dev = _bits(recon)
    for k in range(m):
        assert np.array_equal(dev[k // 3, k % 3], _elements(decoded[k][0], 3, scales[k], biases[k])), k
    # a float16 list of 2-D views with a row window of its own tensor, and the source handed over as a list
    half = _filled((m, SHAPE[2] + 2, SHAPE[3] + 5), 1)
    views = [half[k, 1:1 + SHAPE[2], 3:3 + SHAPE[3]] for k in range(m)]
    got = ctx.encode_batch_from([src[n][c] for n in range(SHAPE[0]) for c in range(SHAPE[1])], scale=SCALE, bias=BIAS, near=nears, effort=efforts,
                                    recon_out=views, recon_scale=0.5, recon_bias=1.0)
    assert got == want
    dev = _bits(half)
    fill = int.from_bytes(bytes([PATTERN]) * 2, "little")
    for k in range(m):
        assert np.array_equal(dev[k, 1:1 + SHAPE[2], 3:3 + SHAPE[3]], _elements(decoded[k][0], 1, 0.5, 1.0)), k
        mask = np.ones(dev[k].shape, bool)
        mask[1:1 + SHAPE[2], 3:3 + SHAPE[3]] = False
        assert (dev[k][mask] == fill).all(), k


def test_a_refused_destination_costs_its_reconstruction_only(ctx, pkg):
    torch = _torch()
    src, planes = _source()
    nears, efforts = _modes(0)
    m = len(planes)
    want = ctx.encode_batch_from(src, scale=SCALE, bias=BIAS, near=nears, effort=efforts)
    decoded = ctx.decode_batch(want)
    for what in ("host", "small", "scale", "none"):
        recon = _filled((m,) + SHAPE[2:], 0 if what != "scale" else 3)
        views = [recon[k] for k in range(m)]
        kw = {}
        cpu = None
        if what == "host":
            cpu = torch.full(SHAPE[2:], PATTERN, dtype=torch.uint8)
            views[1] = views[2] = cpu
        elif what == "small":
            views[1] = recon[1, :SHAPE[2] - 1]
            views[2] = recon[2, :, 1:]
        elif what == "scale":
            kw = dict(recon_scale=[1.0, float("nan"), float("inf"), 1.0, 1.0, 1.0])
        srcs, fmt = pkg._srcs_of(pkg._src_views(src), None, None)
        if what == "none":                                     # the raw call: a null ptr asks for no reconstruction
            dests, rfmt = pkg._dests_ex_of(views, [(s[4], s[5]) for s in srcs], None, None, 1.0, 0.0)
            dests = [(0,) + d[1:] if k in (1, 2) else d for k, d in enumerate(dests)]
            info = {}
            got = ctx.encode_from_srcs(srcs, fmt, SCALE, BIAS, nears, efforts, info=info, recon_dests=dests, recon_fmt=rfmt)
            assert info["rc"] == 0
        else:
            got = ctx.encode_batch_from(src, scale=SCALE, bias=BIAS, near=nears, effort=efforts, recon_out=views, **kw)
        assert got == want, what                               # every stream is written
        assert ctx.deliver_stats() == (m - 2, 0), what
        dev = _bits(recon)
        fill = int.from_bytes(bytes([PATTERN]) * recon.element_size(), "little")
        for k in range(m):
            if k in (1, 2):
                assert (dev[k] == fill).all(), (what, k)
            else:
                assert np.array_equal(dev[k], _elements(decoded[k][0], 3 if what == "scale" else 0, 1.0, 0.0)), (what, k)
        if cpu is not None:
            assert bool((cpu == PATTERN).all())
    # the whole call refused: an unknown format, no destinations; effort 0 and every_rows have no such call
    srcs, fmt = pkg._srcs_of(pkg._src_views(src), None, None)
    dests, _ = pkg._dests_ex_of([_filled(SHAPE[2:], 0)] * m, [(s[4], s[5]) for s in srcs], None, None, 1.0, 0.0)
    with pytest.raises(ValueError):
        ctx.encode_from_srcs(srcs, fmt, SCALE, BIAS, nears, efforts, recon_dests=dests, recon_fmt=4)
    with pytest.raises(ValueError):
        ctx.encode_batch_from(src, scale=SCALE, bias=BIAS, effort=0, recon_out=_filled(SHAPE, 0))
    with pytest.raises(ValueError):
        ctx.encode_batch_from(src, scale=SCALE, bias=BIAS, every_rows=16, recon_out=_filled(SHAPE, 0))
