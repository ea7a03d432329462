"""The band encoder's STAGED front (nblic_amd_stream_set_front, Context.stream(..., front="staged")): lossless -e1 bands on
the key-partitioned kernels of the batch pipeline instead of the one-wave model kernel.  The oracle's stream is the
yardstick; checkpoints and index are held to the serial front's bytes.  Every case is a few thousand pixels, except the
one that needs context chains longer than a block."""
import hashlib

import numpy as np
import pytest

import inputs

gpu = pytest.mark.gpu

# (h, w): smallest image; both rows top rows; no interior column; one 8-pixel run; w = 27; two runs; w = 150; w = 37; long rows
SHAPES = [(1, 1), (2, 7), (9, 19), (9, 20), (17, 27), (17, 28), (23, 150), (40, 37), (5, 5200)]
# 1: a band starts at row 1;  3: bands start at rows 3, 6, ...;  h itself (one band, the whole image) is added per shape
BAND_HEIGHTS = (1, 2, 3, 5)

_oracle_cache = {}


def reference(oracle, content, h, w, seed=None):
    """(image, oracle stream), computed once per plane and shared by the tests."""
    key = (content, h, w, seed)
    if key not in _oracle_cache:
        img = inputs.make(content, h, w) if seed is None else inputs.syn1(h, w, seed)
        want = oracle.encode(img, 0, 1)[0]
        img.setflags(write=False)
        _oracle_cache[key] = (img, want)
    return _oracle_cache[key]


def encode(ctx, img, band, front, index_every=0, per_band=False):
    """The whole image through the band encoder: (stream, sha256 of progress(), reconstruction, index, bands)."""
    enc = ctx.stream(img, 0, 1, band_rows=band, index_every=index_every, front=front)
    try:
        pieces, calls = [], 0
        while True:
            done, b = enc.run(1e-9 if per_band else 0.0)
            pieces.append(b)
            calls += 1
            if done:
                break
        return b"".join(pieces), enc.progress()["sha256"], enc.recon()[0], enc.index(), calls
    finally:
        enc.close()


def band_heights(h):
    return [b for b in BAND_HEIGHTS if b < h] + [h]


@gpu
@pytest.mark.parametrize("h,w", SHAPES)
def test_staged_front_writes_the_oracles_bytes(gpu_ctx, oracle, h, w):
    for content in ("syn1", "noise"):
        img, want = reference(oracle, content, h, w)
        for band in band_heights(h):
            s, sha, rec, _, _ = encode(gpu_ctx, img, band, "staged")
            assert s == want, (content, h, w, band)
            assert sha == hashlib.sha256(want).hexdigest(), (content, h, w, band)
            assert np.array_equal(rec, img), (content, h, w, band)


@gpu
@pytest.mark.parametrize("content,h,w,band", [("const", 40, 300, 14), ("checker", 33, 40, 1), ("checker", 33, 40, 2),
                                              ("checker", 33, 40, 3), ("checker", 33, 40, 5), ("checker", 33, 40, 33)])
def test_staged_front_on_flat_and_alternating_planes(gpu_ctx, oracle, content, h, w, band):
    """const: one context with a constant error -- one chain of 4200 records per band (two blocks) whose warm-up copies
    never meet, so every second block is replayed by the fix-up from a carried state."""
    img, want = reference(oracle, content, h, w)
    s, sha, rec, _, _ = encode(gpu_ctx, img, band, "staged")
    assert s == want
    assert sha == hashlib.sha256(want).hexdigest()
    assert np.array_equal(rec, img)


@gpu
def test_staged_band_with_chains_longer_than_a_block(gpu_ctx, oracle, pkg):
    """131072 pixels per band: the busy contexts' chains run over several 4096-record blocks, warmed up from the extremes
    on top of a carried state."""
    img, want = reference(oracle, "syn1", 256, 2048, seed=1)
    s, _, _, ix, _ = encode(gpu_ctx, img, 64, "staged", index_every=64)
    assert s == want
    assert ix is not None and ix == gpu_ctx.build_index(s, 64)
    assert np.array_equal(gpu_ctx.decode_indexed(s, ix), img)


def one_band(ctx, img, band, front, checkpoint=None):
    """One band in an object of its own: (finished, bytes, checkpoint or None)."""
    enc = ctx.stream(img, 0, 1, band_rows=band, checkpoint=checkpoint, front=front)
    try:
        done, b = enc.run(1e-9)
        return done, b, None if done else enc.checkpoint()
    finally:
        enc.close()


@gpu
@pytest.mark.parametrize("content,h,w,band", [("syn1", 67, 150, 7), ("const", 40, 300, 14), ("syn1", 4, 52000, 2)])
def test_checkpoints_are_the_serial_fronts(gpu_ctx, pkg, oracle, content, h, w, band):
    """After every band the two fronts' checkpoints are the same bytes; then a relay through fresh contexts.  w = 52000:
    rows too wide for the model kernel's LDS, so the encoder keeps a reconstruction and the checkpoint carries two of its
    rows -- which a staged band has to leave there as well."""
    img, want = reference(oracle, content, h, w)
    a = gpu_ctx.stream(img, 0, 1, band_rows=band, front="serial")
    b = gpu_ctx.stream(img, 0, 1, band_rows=band, front="staged")
    try:
        bands = 0
        while True:
            (done_a, bytes_a), (done_b, bytes_b) = a.run(1e-9), b.run(1e-9)
            bands += 1
            assert bytes_a == bytes_b and done_a == done_b, bands
            if done_a:
                break
            ck_a, ck_b = a.checkpoint(), b.checkpoint()
            assert ck_a == ck_b, ("checkpoint after band", bands)
            assert pkg.check_encoder_checkpoint(ck_b)
        assert bands == -(-h // band)
    finally:
        a.close()
        b.close()
    # a relay: every band in a fresh context, resumed from the checkpoint before it, the fronts taking turns
    pieces, ck, k = [], None, 0
    while True:
        ctx = pkg.Context(device=0, n_slots=1, n_coders=1)
        try:
            done, piece, ck = one_band(ctx, img, band, ("staged", "serial")[k % 2], ck)
        finally:
            ctx.close()
        pieces.append(piece)
        k += 1
        if done:
            break
    assert k == -(-h // band)
    assert b"".join(pieces) == want


@gpu
@pytest.mark.parametrize("shape,R,band", [((67, 150), 7, 3), ((23, 150), 1, 4), ((40, 130), 6, 4)])
def test_staged_front_index_is_byte_identical(gpu_ctx, pkg, oracle, shape, R, band):
    h, w = shape
    img, want = reference(oracle, "syn1", h, w, seed=21)
    s, _, _, ix, _ = encode(gpu_ctx, img, band, "staged", index_every=R, per_band=True)
    assert s == want
    assert ix is not None and pkg.check_index(ix, s)
    assert ix == gpu_ctx.build_index(s, R)
    assert np.array_equal(gpu_ctx.decode_indexed(s, ix), img)
    r0 = max(R * ((h // 2) // R) - 1, 0)                                    # from the row above an entry row to two rows below it
    r1 = min(r0 + 3, h)
    assert np.array_equal(gpu_ctx.decode_rows(s, ix, r0, r1), img[r0:r1])


@gpu
def test_it_really_is_the_other_front(gpu_ctx, oracle):
    img, want = reference(oracle, "syn1", 23, 150)
    bands = -(-23 // 4)
    n0 = gpu_ctx.serial_launches()
    enc = gpu_ctx.stream(img, 0, 1, band_rows=4, front="staged")
    try:
        assert enc.front == "staged"
        while not enc.run()[0]:
            pass
        assert enc.progress()["model_kernel_ms"] > 0
    finally:
        enc.close()
    assert gpu_ctx.serial_launches() == n0
    enc = gpu_ctx.stream(img, 0, 1, band_rows=4)
    try:
        assert enc.front == "serial"
        while not enc.run()[0]:
            pass
        assert enc.progress()["model_kernel_ms"] > 0
    finally:
        enc.close()
    assert gpu_ctx.serial_launches() == n0 + bands


@gpu
def test_refusals_launch_nothing_and_leak_nothing(pkg, oracle):
    img, want = reference(oracle, "syn1", 23, 150)
    ctx = pkg.Context(device=0, n_slots=1, n_coders=1)
    try:
        for front in ("serial", "staged"):                                  # the group's workspace is as large as it will get
            assert encode(ctx, img, 4, front)[0] == want
        live, launches = pkg.live_resources(), ctx.serial_launches()
        for near, effort in ((1, 1), (0, 2), (2, 3)):
            with pytest.raises(RuntimeError):
                ctx.stream(img, near, effort, band_rows=4, front="staged")
        with pytest.raises(RuntimeError):
            ctx.stream(img, 0, 1, band_rows=4, front="bogus")
        lib = ctx.lib
        assert lib.nblic_amd_stream_set_front(None, 1) == -1 and lib.nblic_amd_stream_set_front(None, 0) == -1
        enc = ctx.stream(img, 0, 1, band_rows=4)
        try:
            assert lib.nblic_amd_stream_set_front(enc.handle, 2) == -1 and lib.nblic_amd_stream_set_front(enc.handle, -1) == -1
            assert lib.nblic_amd_stream_set_front(enc.handle, 1) == 0 and lib.nblic_amd_stream_set_front(enc.handle, 0) == 0
            done, first = enc.run(1e-9)
            assert not done
            assert lib.nblic_amd_stream_set_front(enc.handle, 1) == -1      # after the first _run
            assert lib.nblic_amd_stream_set_front(enc.handle, 0) == -1
            rest = b""
            while not done:
                done, b = enc.run()
                rest += b
            assert first + rest == want
        finally:
            enc.close()
        assert ctx.serial_launches() == launches + -(-23 // 4)              # that serial encode alone: no refusal launched
        assert pkg.live_resources() == live
        s, *_ = encode(ctx, img, 4, "staged")                               # the refused context still encodes: its group came back
        assert s == want
        assert pkg.live_resources() == live
    finally:
        ctx.close()


def test_set_front_refuses_null_without_a_device(pkg):
    lib = pkg.load_library()
    assert lib.nblic_amd_stream_set_front(None, 1) == -1
    assert lib.nblic_amd_stream_set_front(None, 0) == -1


def test_set_front_is_declared(pkg):
    text = open(pkg.INCLUDE).read()
    assert "int nblic_amd_stream_set_front(nblic_amd_stream *s, int front);" in text
    assert "nblic_amd_stream_set_front" in pkg.EXPORTS
    assert pkg.FRONTS == {"serial": 0, "staged": 1}
