"""GPU suite (-m gpu): every HIP resource the host side takes comes back.  The owners of csrc/hip_owned.h count what is
live (pkg.live_resources(): device allocations, runtime-pinned allocations, page-locked host buffers, streams + events);
each test takes a reading, works on a Context of its own -- batch paths with growth, band and index paths, failure
paths -- closes it and requires the same reading.  The shapes are tiny: the subject is the host side.  Neither the
session's gpu_ctx nor the default context is touched between two readings (their buffers grow lazily)."""
import contextlib
import gc

import numpy as np
import pytest

import inputs
from test_seek_index import _join, _reseal_entry, _split

pytestmark = pytest.mark.gpu

MODES = [(0, 1), (2, 2), (0, 3)]
SMALL, LARGE, BAND = (16, 24), (40, 56), (18, 32)


@pytest.fixture(scope="module")
def refs(oracle):
    """The oracle's streams and reconstructions, computed once: refs[(h, w)] = (image, {(near, effort): (stream, recon)},
    QNBLIC stream)."""
    out = {}
    for k, (h, w) in enumerate((SMALL, LARGE, BAND)):
        img = inputs.syn1(h, w, 3 + k)
        out[(h, w)] = (img, {m: oracle.encode(img, *m)[:2] for m in MODES}, oracle.qencode(img))
    return out


@contextlib.contextmanager
def accounted(pkg):
    """A context of the test's own between two readings that must agree; while it is open the library must hold more."""
    gc.collect()
    before = pkg.live_resources()
    ctx = pkg.Context(device=0, n_slots=2, n_coders=2)
    try:
        yield ctx
        during = pkg.live_resources()
        assert during["device"] > before["device"] and during["streams_events"] > before["streams_events"], (before, during)
    finally:
        ctx.close()
    gc.collect()
    assert pkg.live_resources() == before


def test_batch_paths_with_growth(pkg, refs):
    with accounted(pkg) as ctx:
        streams, want = [], []
        for shape in (SMALL, LARGE, SMALL):                              # grow every pixel- and event-sized buffer, then nothing shrinks
            img, by_mode, _ = refs[shape]
            got, recs = ctx.encode_modes([img] * len(MODES), [m[0] for m in MODES], [m[1] for m in MODES])
            for m, s, r in zip(MODES, got, recs):
                assert s == by_mode[m][0], (shape, m)
                assert np.array_equal(r, by_mode[m][1]), (shape, m)
            streams += got
            want += [by_mode[m][1] for m in MODES]
        q = ctx.qencode_batch([refs[SMALL][0], refs[LARGE][0]])
        assert q == [refs[SMALL][2], refs[LARGE][2]]
        streams += q
        want += [refs[SMALL][0], refs[LARGE][0]]
        planes = ctx.decode_batch(streams)
        assert all(p is not None and np.array_equal(p[0], w) for p, w in zip(planes, want))


def test_band_and_index_paths(pkg, refs):
    img, by_mode, q = refs[BAND]
    want, rec = by_mode[(2, 2)]
    with accounted(pkg) as ctx:
        a = ctx.stream(img, 2, 2, band_rows=4, index_every=8)
        done, head = a.run(1e-9)                                         # one band, then the budget is spent
        assert not done and head
        ck = a.checkpoint()
        done, tail = a.run()
        assert done and head + tail == want
        index = a.index()
        a.close()
        b = ctx.stream(img, 2, 2, checkpoint=ck)
        done, tail = b.run()
        assert done and head + tail == want
        b.close()
        for stream, plane in ((want, rec), (q, img)):
            assert np.array_equal(pkg.decompress_bands(stream, band_rows=4, chunk=50, ctx=ctx), plane)
            ix = ctx.build_index(stream, 8)
            assert stream is not want or ix == index
            ctx.set_index_round(1)                                       # three segments, three rounds
            assert np.array_equal(ctx.decode_indexed(stream, ix), plane)
            ctx.set_index_round(0)
            assert np.array_equal(ctx.decode_rows(stream, ix, 5, 11), plane[5:11])


def test_failure_paths_give_everything_back(pkg, oracle, refs):
    img, by_mode, _ = refs[BAND]
    want, rec = by_mode[(2, 2)]
    other = oracle.encode(inputs.syn1(BAND[0], BAND[1], 11), 2, 2)[0]
    with accounted(pkg) as ctx:
        with pytest.raises(RuntimeError):                                # the output does not even hold the header
            ctx.encode_ptrs([img.ctypes.data], [img.shape], False, outs=[np.empty(64, np.uint8)[:8]])
        s = ctx.stream(img, 2, 2, band_rows=4)
        assert not s.run(1e-9)[0]
        ck = bytearray(s.checkpoint())
        s.close()
        ck[len(ck) // 2] ^= 0x10
        with pytest.raises(RuntimeError):
            ctx.stream(img, 2, 2, checkpoint=bytes(ck))
        ix = ctx.build_index(want, 8)
        with pytest.raises(RuntimeError):                                # another stream's index: refused at the stream hash
            ctx.decode_indexed(want, ctx.build_index(other, 8))
        head, ents = _split(ix)
        e = bytearray(ents[1])
        e[len(e) - 32 - 2 * BAND[1] + BAND[1] + 17] ^= 0x01              # a row above the entry: each check of the entry alone passes
        forged = _join(head, [ents[0], _reseal_entry(bytes(e))])
        assert pkg.check_index(forged, want)
        with pytest.raises(RuntimeError):                                # refused by the chain check, after the launches
            ctx.decode_indexed(want, forged)
        assert np.array_equal(ctx.decode_indexed(want, ix), rec)
        assert ctx.decode_batch([want[:40]]) == [None]
        s = ctx.stream(img, 2, 2, band_rows=4)                           # dropped without close(), mid-image
        assert not s.run(1e-9)[0]
        d = ctx.decoder(4)
        d.feed(want[:len(want) // 2])
        assert d.run()[0] == pkg.NEEDS_INPUT
        del s, d
        gc.collect()


def test_drop_in_entry_points_hold_nothing_per_call(pkg, refs):
    img, by_mode, _ = refs[SMALL]

    def once():
        s, rec, _, _ = pkg.compress(img, 2, 2)
        assert s == by_mode[(2, 2)][0] and np.array_equal(rec, by_mode[(2, 2)][1])
        assert np.array_equal(pkg.decompress(s)[0], rec)

    once()                                                               # creates the default context, grows its buffers
    before = pkg.live_resources()
    assert before["device"] > 0 and before["streams_events"] > 0
    for _ in range(10):
        once()
    assert pkg.live_resources() == before                                # decode_dropin's band decoder came and went each time
