"""The indexed batch (nblic_amd_encode_batch_indexed, Context.encode_batch_indexed): a group of lossless -e1 images stepped
through row bands together, streams and seek indexes out.  The oracle's stream is the yardstick for the bytes, the serial
index builder (Context.build_index) for the indexes.  The shapes are the band front's (test_band_front.py): the smallest at
which its kernels take another path; here several of them share every launch, at different rows."""
import threading

import numpy as np
import pytest

import inputs

gpu = pytest.mark.gpu

SHAPES = [(1, 1), (2, 7), (9, 19), (9, 20), (17, 27), (17, 28), (23, 150), (40, 37), (5, 5200)]
_cache = {}


def reference(oracle, content, h, w, seed=None):
    """(image, oracle stream), computed once per plane and shared by the tests."""
    key = (content, h, w, seed)
    if key not in _cache:
        img = inputs.make(content, h, w) if seed is None else inputs.syn1(h, w, seed)
        want = oracle.encode(img, 0, 1)[0]
        img.setflags(write=False)
        _cache[key] = (img, want)
    return _cache[key]


@pytest.fixture
def ctx1(pkg, gpu_ctx):
    ctx = pkg.Context(device=0, n_slots=4, n_coders=2, n_groups=1)
    yield ctx
    ctx.close()


def check(pkg, gpu_ctx, got, refs, every):
    """Every (stream, index) of `got` against the oracle's stream and the serial builder's index."""
    assert len(got) == len(refs)
    for k, ((s, ix), (img, want), r) in enumerate(zip(got, refs, every)):
        h, w = img.shape
        assert s == want, (k, h, w, r)
        if r < 1 or r >= h:
            assert ix is None, (k, h, w, r)
            continue
        assert ix is not None and len(ix) == pkg.index_bytes(0, h, w, 1, r), (k, h, w, r)
        assert ix == gpu_ctx.build_index(s, r), (k, h, w, r)
        assert np.array_equal(gpu_ctx.decode_indexed(s, ix), img), (k, h, w, r)


@gpu
@pytest.mark.parametrize("content", ["syn1", "noise"])
def test_all_shapes_in_one_call(pkg, gpu_ctx, ctx1, oracle, content):
    """Nine images on four slots: slots are refilled, and jobs at different rows and of different widths share launches."""
    refs = [reference(oracle, content, h, w) for h, w in SHAPES]
    every = [(1, 2, 3, 5)[k % 4] for k in range(len(refs))]
    before = ctx1.serial_launches()
    got = ctx1.encode_batch_indexed([r[0] for r in refs], every)
    assert ctx1.serial_launches() == before                               # no serial kernel is involved
    check(pkg, gpu_ctx, got, refs, every)


@gpu
@pytest.mark.parametrize("band", [2, 3])
def test_bands_that_do_not_divide_every_rows(pkg, gpu_ctx, ctx1, oracle, band):
    refs = [reference(oracle, "syn1", 23, 150), reference(oracle, "syn1", 40, 37)]
    before = ctx1.serial_launches()
    got = ctx1.encode_batch_indexed([r[0] for r in refs], 5, band_rows=band)
    assert ctx1.serial_launches() == before
    check(pkg, gpu_ctx, got, refs, [5, 5])
    for (s, ix), (img, _) in zip(got, refs):                              # the band encoder, one image per object
        enc = gpu_ctx.stream(img, 0, 1, band_rows=band, index_every=5, front="staged")
        try:
            done, alone = enc.run(0.0)
            assert done and alone == s
            assert enc.index() == ix
        finally:
            enc.close()


@gpu
def test_carried_state_in_the_fixup_path(pkg, gpu_ctx, ctx1, oracle):
    """const: one context chain of 4200 records per 14-row band, two blocks, the second replayed by the fix-up from a carried
    state -- next to a checker and a syn1 plane in the same launches."""
    refs = [reference(oracle, "const", 40, 300), reference(oracle, "checker", 33, 40), reference(oracle, "syn1", 23, 150)]
    every = [14, 5, 7]
    before = ctx1.serial_launches()
    got = ctx1.encode_batch_indexed([r[0] for r in refs], every)
    assert ctx1.serial_launches() == before
    check(pkg, gpu_ctx, got, refs, every)


@gpu
def test_chains_longer_than_a_block_in_several_jobs(pkg, gpu_ctx, ctx1, oracle):
    """131072 pixels per band and job: chains over several 4096-record blocks, in three jobs of one launch."""
    refs = [reference(oracle, "syn1", 256, 2048, seed=1), reference(oracle, "syn1", 256, 2048, seed=2), reference(oracle, "syn1", 64, 2048, seed=3)]
    before = ctx1.serial_launches()
    got = ctx1.encode_batch_indexed([r[0] for r in refs], 64)
    assert ctx1.serial_launches() == before
    assert got[2][1] is None                                              # 64 rows, R = 64: no entry row
    check(pkg, gpu_ctx, got, refs, [64, 64, 64])


@gpu
def test_more_images_than_slots_on_two_groups(pkg, gpu_ctx, oracle):
    shapes = [(3 + (37 * k) // 10, 20 + 13 * k) for k in range(11)]       # heights 3 .. 40, widths 20 .. 150
    assert shapes[0] == (3, 20) and shapes[-1] == (40, 150)
    refs = [reference(oracle, "syn1", h, w) for h, w in shapes]
    ctx = pkg.Context(device=0, n_slots=4, n_coders=2, n_groups=2)
    try:
        before = ctx.serial_launches()
        got = ctx.encode_batch_indexed([r[0] for r in refs], 4)
        assert ctx.serial_launches() == before
    finally:
        ctx.close()
    check(pkg, gpu_ctx, got, refs, [4] * len(refs))


@gpu
def test_device_resident_inputs(pkg, gpu_ctx, ctx1, oracle):
    import torch
    refs = [reference(oracle, "syn1", h, w) for h, w in ((9, 20), (23, 150), (5, 5200))]
    every = [2, 5, 1]
    host = ctx1.encode_batch_indexed([r[0] for r in refs], every)
    tensors = [torch.from_numpy(np.array(r[0])).cuda() for r in refs]
    torch.cuda.synchronize()
    dev = ctx1.encode_batch_indexed(tensors, every)
    assert dev == host
    check(pkg, gpu_ctx, dev, refs, every)


@gpu
def test_failures_stay_local_and_nothing_leaks(pkg, gpu_ctx, oracle):
    refs = [reference(oracle, "syn1", h, w) for h, w in ((9, 20), (17, 28), (23, 150), (40, 37), (17, 27))]
    planes = [np.ascontiguousarray(r[0]) for r in refs]
    ptrs, shapes = [p.ctypes.data for p in planes], [p.shape for p in planes]
    every = [2, 3, 5, 4, 2]
    outside = pkg.live_resources()
    ctx = pkg.Context(device=0, n_slots=4, n_coders=2, n_groups=1)
    try:
        rc, streams, indexes = ctx.encode_indexed_ptrs(ptrs, shapes, False, every)     # the slots' band workspaces are the context's: grown here
        assert rc == 0
        check(pkg, gpu_ctx, list(zip(streams, indexes)), refs, every)
        before, launches = pkg.live_resources(), ctx.serial_launches()
        out_caps = [pkg.out_capacity(h, w) for h, w in shapes]
        index_caps = [pkg.index_bytes(0, h, w, 1, r) for (h, w), r in zip(shapes, every)]
        out_caps[1] = 8
        index_caps[3] = 8
        rc, s2, x2 = ctx.encode_indexed_ptrs(ptrs, shapes, False, every, out_caps=out_caps, index_caps=index_caps)
        assert rc == -1
        assert pkg.live_resources() == before
        assert s2[1] is None and x2[1] is None and x2[3] is None
        assert s2[3] == refs[3][1]                                        # the stream of the image with the small index buffer
        for k in (0, 2, 4):
            assert s2[k] == streams[k] and x2[k] == indexes[k], k
        # a negative every_rows refuses the whole call: nothing launched, nothing allocated
        k = len(ptrs)
        imgs, hs, ws, op, caps, lens = pkg._batch_args(ptrs, shapes, [np.empty(c, np.uint8) for c in [pkg.out_capacity(h, w) for h, w in shapes]])
        import ctypes as C
        rc = ctx.lib.nblic_amd_encode_batch_indexed(ctx.handle, k, imgs, 0, hs, ws, (C.c_int * k)(2, 3, -1, 4, 2), 0, op, caps, lens, None, None, None)
        assert rc == -1
        assert pkg.live_resources() == before and ctx.serial_launches() == launches
        rc, s3, x3 = ctx.encode_indexed_ptrs(ptrs, shapes, False, every)  # and the context still works
        assert rc == 0 and s3 == streams and x3 == indexes
        assert pkg.live_resources() == before and ctx.serial_launches() == launches
    finally:
        ctx.close()
    assert pkg.live_resources() == outside


@gpu
def test_next_to_a_plain_batch(pkg, gpu_ctx, oracle):
    a = [reference(oracle, "syn1", h, w) for h, w in ((9, 20), (17, 27), (17, 28), (23, 150), (40, 37), (9, 19))]
    b = [reference(oracle, "noise", h, w) for h, w in ((9, 20), (17, 27), (17, 28), (23, 150), (40, 37), (9, 19))]
    ctx = pkg.Context(device=0, n_slots=4, n_coders=2, n_groups=2)
    result = {}

    def indexed():
        try:
            result["got"] = ctx.encode_batch_indexed([r[0] for r in a], 4)
        except Exception as e:                                            # noqa: BLE001 -- reported by the main thread
            result["error"] = e

    try:
        before = ctx.serial_launches()
        t = threading.Thread(target=indexed)
        t.start()
        plain = ctx.encode_batch([r[0] for r in b])
        t.join()
        assert ctx.serial_launches() == before
    finally:
        ctx.close()
    assert "error" not in result, result.get("error")
    assert plain == [r[1] for r in b]
    check(pkg, gpu_ctx, result["got"], a, [4] * len(a))
