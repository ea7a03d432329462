"""GPU suite (-m gpu): the packed seek index on the device.  pack_index of a real index unpacks to the same bytes and is
strictly smaller; decode_batch_indexed expands it with k_index_unpack and returns the planes and row ranges the unpacked
index gives -- every mode, odd widths, the longest chain (64 entries) and a single entry, rounds that start above segment 0,
packed and unpacked indexes mixed in one call, a damaged one refused alone.  The images are the smallest at which the kernel
takes every path: B (8-byte units, fields across three words) at efforts 2 / 3, the row slot ending in a short unit (odd W),
doubles at 4 mod 8 (W = 2 mod 4), entries walked but not stored (rounds, row ranges)."""
import hashlib
import struct

import numpy as np
import pytest

import inputs
from test_seek_index import _stream

pytestmark = pytest.mark.gpu

MODES = [("n", 0, 1), ("n", 3, 1), ("n", 0, 2), ("n", 2, 3), ("q", 0, 0)]
SIZES = [(37, 29, 5), (38, 30, 5), (65, 64, 1), (24, 20, 19)]                  # (h, w, R): odd W; W = 2 mod 4; 64 entries; one entry

_cache = {}


def _made(gpu_ctx, oracle):
    """{(mode, size): (stream, index, reconstruction)}: every stream once, every index from ONE build_index_batch call."""
    if not _cache:
        keys = [(m, g) for m in MODES for g in SIZES]
        streams = [_stream(oracle, *m, g[0], g[1]) for m, g in keys]
        indexes = gpu_ctx.build_index_batch([s for s, _ in streams], [g[2] for _, g in keys])
        for key, (s, rec), ix in zip(keys, streams, indexes):
            assert ix is not None, key
            _cache[key] = (s, ix, rec)
    return _cache


class _live:
    """nblic_amd_debug_live must return to what it was before the calls inside."""
    def __init__(self, pkg):
        self.pkg = pkg

    def __enter__(self):
        self.before = self.pkg.live_resources()

    def __exit__(self, *exc):
        if exc[0] is None:
            assert self.pkg.live_resources() == self.before, "a call on a packed index kept a device resource"


@pytest.mark.parametrize("mode", MODES)
def test_every_mode_and_size(gpu_ctx, pkg, oracle, mode):
    made = _made(gpu_ctx, oracle)
    cases = [made[(mode, g)] for g in SIZES]
    packed = []
    for (s, ix, _), g in zip(cases, SIZES):
        p = pkg.pack_index(ix)
        assert pkg.index_is_packed(p) and pkg.check_index(p, s), g
        assert pkg.unpack_index(p) == ix, g
        assert len(p) < len(ix), g
        print(f"packed index {mode} {g}: {len(ix)} -> {len(p)} bytes (stream {len(s)})")
        packed.append(p)
    plain = gpu_ctx.decode_batch([s for s, _, _ in cases])
    with _live(pkg):
        info = {}
        planes = gpu_ctx.decode_batch_indexed([(s, p) for (s, _, _), p in zip(cases, packed)], info=info)
    assert info["rc"] == 0 and info["status"] == [0] * len(cases)
    for (s, ix, rec), plane, whole, g in zip(cases, planes, plain, SIZES):
        assert plane is not None and np.array_equal(plane, whole[0]), g
        assert np.array_equal(plane, rec), g


def _damaged(packed):
    """A packed index with one payload bit flipped and the outer seal made right: the entry's own hash refuses it."""
    b = bytearray(packed)
    b[128 + 8 + 168 + 300] ^= 0x10
    return bytes(b[:-32]) + hashlib.sha256(bytes(b[:-32])).digest()


def test_packed_and_unpacked_mixed_one_damaged(gpu_ctx, pkg, oracle):
    made = _made(gpu_ctx, oracle)
    keys = [(m, g) for m in MODES for g in SIZES[:2] + SIZES[3:]]
    pairs, want = [], []
    for k, key in enumerate(keys):
        s, ix, rec = made[key]
        pairs.append((s, pkg.pack_index(ix) if k % 2 == 0 else ix))
        want.append(rec)
    bad = 4
    assert pkg.index_is_packed(pairs[bad][1])
    pairs[bad] = (pairs[bad][0], _damaged(pairs[bad][1]))
    assert not pkg.check_index(pairs[bad][1])
    with _live(pkg):
        info = {}
        planes = gpu_ctx.decode_batch_indexed(pairs, info=info)
    assert info["rc"] == -1 and info["status"] == [-1 if k == bad else 0 for k in range(len(pairs))]
    for k, (plane, rec) in enumerate(zip(planes, want)):
        if k == bad:
            assert plane is None
        else:
            assert plane is not None and np.array_equal(plane, rec), keys[k]


def test_row_ranges_and_rounds_that_start_above_segment_0(gpu_ctx, pkg, oracle):
    made = _made(gpu_ctx, oracle)
    pairs, rows, want = [], [], []
    for mode in MODES:
        for g in SIZES[:3]:
            h, w, R = g
            s, ix, rec = made[(mode, g)]
            p = pkg.pack_index(ix)
            last = ((h - 1) // R) * R                                          # the last segment's first row
            mid = ((h - 1) // R // 2) * R
            for r in ((0, 1), (1, min(h, 2 * R + 1)), (mid, mid + 1), (mid - 1, min(h, mid + R + 1)), (last, h), (last - 1, h), (0, h)):
                pairs.append((s, p)); rows.append(r); want.append(rec[r[0]:r[1]])          # the oracle's rows
                assert np.array_equal(gpu_ctx.decode_rows(s, ix, *r), want[-1])
    gpu_ctx.set_index_round(3)                                                 # rounds start at s0 > 0: the walk from entry 0 stores from s0 on
    try:
        with _live(pkg):
            got = gpu_ctx.decode_batch_indexed(pairs, rows)
            whole = gpu_ctx.decode_batch_indexed([(made[(m, SIZES[2])][0], pkg.pack_index(made[(m, SIZES[2])][1])) for m in MODES])
    finally:
        gpu_ctx.set_index_round(0)
    for g, wnt, r in zip(got, want, rows):
        assert g is not None and np.array_equal(g, wnt), r
    for m, plane in zip(MODES, whole):
        assert plane is not None and np.array_equal(plane, made[(m, SIZES[2])][2]), m
    with _live(pkg):
        got = gpu_ctx.decode_batch_indexed(pairs, rows)                        # and in one round
    for g, wnt, r in zip(got, want, rows):
        assert g is not None and np.array_equal(g, wnt), r


def test_single_image_paths_take_a_packed_index(gpu_ctx, pkg, oracle):
    made = _made(gpu_ctx, oracle)
    for mode in MODES:
        s, ix, rec = made[(mode, SIZES[0])]
        p = pkg.pack_index(ix)
        with _live(pkg):
            assert np.array_equal(gpu_ctx.decode_indexed(s, p), rec), mode
            assert np.array_equal(gpu_ctx.decode_rows(s, p, 11, 23), rec[11:23]), mode
        with pytest.raises(RuntimeError):
            gpu_ctx.decode_indexed(s, _damaged(p))
        with pytest.raises(RuntimeError):
            gpu_ctx.decode_rows(s, _damaged(p), 11, 23)


def test_indexes_of_the_write_paths(gpu_ctx, pkg, oracle):
    """The band encoder's index and the indexed batch encode's: each packs, unpacks to itself and decodes."""
    img = inputs.syn1(37, 29, 9)
    enc = gpu_ctx.stream(img, 2, 2, band_rows=4, index_every=5)
    try:
        done, s = enc.run(0.0)
        assert done
        band_ix = enc.index()
    finally:
        enc.close()
    rec = oracle.encode(img, 2, 2)[1]
    (bs, batch_ix), = gpu_ctx.encode_batch_indexed([img], 5)
    pairs, want = [], []
    for stream, ix, plane in ((s, band_ix, rec), (bs, batch_ix, img)):
        assert ix is not None and pkg.check_index(ix, stream)
        p = pkg.pack_index(ix)
        assert pkg.unpack_index(p) == ix and len(p) < len(ix) and pkg.check_index(p, stream)
        pairs.append((stream, p)); want.append(plane)
    with _live(pkg):
        planes = gpu_ctx.decode_batch_indexed(pairs)
    for plane, wnt in zip(planes, want):
        assert plane is not None and np.array_equal(plane, wnt)
