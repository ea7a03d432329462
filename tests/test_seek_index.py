"""GPU suite (-m gpu): the seek index (nblic_amd_index_*, nblic_amd_decode_indexed / _rows).  An index built from a stream
decodes the image as segments side by side and any row range on its own; every plane must equal the oracle's, bit for
bit, and every damaged or foreign index must be refused before anything is launched."""
import ctypes as C
import hashlib
import struct
import threading
import time

import numpy as np
import pytest

import inputs

pytestmark = pytest.mark.gpu

CASES = [("n", 0, 1), ("n", 2, 1), ("n", 0, 2), ("n", 3, 3), ("q", 0, 0)]
GEOMS = [(23, 150), (67, 150)]


def _stream(oracle, kind, near, effort, h, w, seed=5):
    img = inputs.syn1(h, w, seed)
    if kind == "q":
        return oracle.qencode(img), img
    s, rec, *_ = oracle.encode(img, near, effort)
    return s, rec


def _split(ix):
    """(head, [entries]) of an index, without checking it."""
    count = struct.unpack_from("<i", ix, 40)[0]
    at, ents = 96, []
    for _ in range(count):
        n = struct.unpack_from("<Q", ix, at)[0]
        ents.append(ix[at + 8:at + 8 + n])
        at += 8 + n
    return ix[:96], ents


def _join(head, ents):
    body = head + b"".join(struct.pack("<Q", len(e)) + e for e in ents)
    return body + hashlib.sha256(body).digest()


def _reseal_entry(e):
    return e[:-32] + hashlib.sha256(e[:-32]).digest()


@pytest.mark.parametrize("kind,near,effort", CASES)
def test_indexed_and_row_range_decodes_match_the_oracle(gpu_ctx, pkg, oracle, kind, near, effort):
    for h, w in GEOMS:
        s, rec = _stream(oracle, kind, near, effort, h, w)
        for R in (1, 3, 7):
            ix = gpu_ctx.build_index(s, R)
            assert pkg.check_index(ix, s), (h, R)
            ents = pkg.index_entries(ix)
            assert len(ents) == (h - 1) // R
            assert np.array_equal(gpu_ctx.decode_indexed(s, ix), rec), (kind, near, effort, h, R)
            k = len(ents) // 2 + 1
            for r0 in sorted({k * R, k * R - 1, k * R + 1, 0, h - 1}):
                assert np.array_equal(gpu_ctx.decode_rows(s, ix, r0, h), rec[r0:]), (h, R, r0)
                assert np.array_equal(gpu_ctx.decode_rows(s, ix, r0, r0 + 1), rec[r0:r0 + 1]), (h, R, r0)
            assert np.array_equal(gpu_ctx.decode_rows(s, ix, 1, h - 1), rec[1:h - 1])
            # every entry resumes a band decoder that finishes the image
            for i, e in enumerate(ents):
                d = gpu_ctx.decoder(checkpoint=e)
                ff = d.progress()["feed_from"]
                d.feed(s[ff:], final=True)
                rc, rows, first = d.run()
                d.close()
                assert rc == 1 and first == (i + 1) * R and np.array_equal(rows, rec[first:]), (h, R, i)


ENC_CASES = [(0, 1), (2, 1), (0, 2), (3, 3)]


@pytest.mark.parametrize("near,effort", ENC_CASES)
def test_band_encoder_index_is_byte_identical(gpu_ctx, pkg, oracle, near, effort):
    """The band encoder's index (state converted to the decoder's records as it codes) against build_index of the stream
    it wrote, with band heights that do not divide R: byte for byte."""
    for (h, w), R, band in (((67, 150), 7, 3), ((23, 150), 1, 4), ((40, 130), 6, 4)):
        img = inputs.syn1(h, w, 21)
        want, rec, *_ = oracle.encode(img, near, effort)
        enc = gpu_ctx.stream(img, near, effort, band_rows=band, index_every=R)
        pieces = []
        while True:
            done, b = enc.run(budget_seconds=1e-6)          # a call per band: entries wait across calls for their window
            pieces.append(b)
            if done:
                break
        s = b"".join(pieces)
        ix = enc.index()
        enc.close()
        assert s == want, (near, effort, h, R)
        assert ix is not None and pkg.check_index(ix, s)
        assert ix == gpu_ctx.build_index(s, R), (near, effort, h, R, band)
        assert np.array_equal(gpu_ctx.decode_indexed(s, ix), rec)


def test_band_encoder_index_refusals(gpu_ctx, oracle):
    img = inputs.syn1(30, 80, 22)
    for R in (-1, 30, 31):                                  # (index_every=0 in Python: no index asked for)
        with pytest.raises(RuntimeError):
            gpu_ctx.stream(img, 0, 1, band_rows=4, index_every=R)
    enc = gpu_ctx.stream(img, 0, 1, band_rows=4)
    assert enc.lib.nblic_amd_stream_set_index(enc.handle, 0) == -1
    done, first = enc.run(budget_seconds=1e-6)
    assert not done and enc.index() is None                 # never asked for one
    ck = enc.checkpoint()
    enc.close()
    res = gpu_ctx.stream(img, 0, 1, checkpoint=ck)
    assert res.lib.nblic_amd_stream_set_index(res.handle, 5) == -1      # a resumed encoder cannot index the rows it did not code
    while not res.run()[0]:
        pass
    assert res.index() is None
    res.close()


def test_indexed_decode_in_several_rounds(gpu_ctx, oracle):
    """Rounds of 2 and 3 segments: the job list (indexed_decode_plan) names an image's segments from the last to the first
    and is cut into rounds in that order, and each segment's rows must end as that segment decoded them."""
    try:
        for kind, near, effort in CASES:
            s, rec = _stream(oracle, kind, near, effort, 67, 150)
            ix = gpu_ctx.build_index(s, 7)                  # 10 segments
            for per_round in (2, 3):
                gpu_ctx.set_index_round(per_round)
                assert np.array_equal(gpu_ctx.decode_indexed(s, ix), rec), (kind, near, effort, per_round)
            _, ents = _split(ix)
            e = bytearray(ents[5])
            e[len(e) - 32 - 2 * 150 - (24576 if kind == "q" else 0) + 3] ^= 0x04      # a row above entry 6 (row 42), resealed
            forged = _join(ix[:96], ents[:5] + [_reseal_entry(bytes(e))] + ents[6:])
            gpu_ctx.set_index_round(2)                      # the plan's rounds: segments 9 8 | 7 6 | 5 4 | ...: the boundary in front of row 42 lies between two rounds
            with pytest.raises(RuntimeError):
                gpu_ctx.decode_indexed(s, forged)
    finally:
        gpu_ctx.set_index_round(0)


def test_refused_result_leaves_no_pixels(gpu_ctx, oracle):
    s, rec = _stream(oracle, "n", 0, 1, 30, 100, seed=9)
    ix = gpu_ctx.build_index(s, 10)
    head, ents = _split(ix)
    e = bytearray(ents[1])
    e[len(e) - 32 - 2 * 100 + 150] ^= 0x01
    forged = _join(head, [ents[0], _reseal_entry(bytes(e))])
    sb, xb = np.frombuffer(s, np.uint8).copy(), np.frombuffer(forged, np.uint8).copy()
    out = np.full(30 * 100, 0x5A, np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert gpu_ctx.lib.nblic_amd_decode_indexed(gpu_ctx.handle, p(sb), sb.size, p(xb), xb.size, p(out), out.size) == -1
    assert not out.any()


def test_every_golden_stream_through_an_index(gpu_ctx, golden, oracle):
    """All 500 small golden streams: build_index + decode_indexed to the golden reconstruction hash (QNBLIC: the oracle's
    plane).  A one-row image has no row to index and is refused."""
    manifest, streams = golden
    n = 0
    for key in streams.keys():
        s = streams[key].tobytes()
        if s[:1] == b"Q":
            want_sha = hashlib.sha256(oracle.qdecode(s).tobytes()).hexdigest()
            h = int.from_bytes(s[4:6], "little")
        else:
            want_sha = manifest["small"][key]["recon_sha256"]
            h = (s[9] << 8) | s[10]
        if h < 2:
            with pytest.raises(RuntimeError):
                gpu_ctx.build_index(s, 1)
            continue
        R = max(1, h // 4)
        ix = gpu_ctx.build_index(s, R)
        plane = gpu_ctx.decode_indexed(s, ix)
        assert hashlib.sha256(plane.tobytes()).hexdigest() == want_sha, (key, R)
        n += 1
    assert n >= 400


def test_refusals_before_any_launch(gpu_ctx, pkg, oracle):
    h, w = 40, 130
    s, rec = _stream(oracle, "n", 0, 2, h, w, seed=7)
    other, _ = _stream(oracle, "n", 0, 2, h, w, seed=8)
    assert len(other) > 0 and other[:16] == s[:16]
    ix = gpu_ctx.build_index(s, 6)
    head, ents = _split(ix)
    flips = []
    for at in (20, 60, 96 + 8 + 40, 96 + 8 + 5000, len(ix) - 40, len(ix) - 1):   # head, an entry's head and body, the last entry, the trailer
        b = bytearray(ix)
        b[at] ^= 0x10
        flips.append(bytes(b))
    bad_ixs = flips + [ix[:-1], ix[:len(ix) // 2], ix[:96]]
    lib = gpu_ctx.lib
    before = gpu_ctx.serial_launches()
    with pytest.raises(RuntimeError):
        gpu_ctx.decode_indexed(other, ix)                       # another stream of the same geometry and mode
    with pytest.raises(RuntimeError):
        gpu_ctx.decode_rows(other, ix, 10, 20)
    for b in bad_ixs:
        assert not pkg.check_index(b)
        with pytest.raises(RuntimeError):
            gpu_ctx.decode_indexed(s, b)
        with pytest.raises(RuntimeError):
            gpu_ctx.decode_rows(s, b, 7, 9)
    for r in (0, -3, h, h + 1):
        with pytest.raises(RuntimeError):
            gpu_ctx.build_index(s, r)
    for r0, r1 in ((5, 5), (6, 3), (-1, 4), (0, h + 1)):
        with pytest.raises(RuntimeError):
            gpu_ctx.decode_rows(s, ix, r0, r1)
    sb = np.frombuffer(s, np.uint8).copy()
    xb = np.frombuffer(ix, np.uint8).copy()
    out = np.zeros(h * w, np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.nblic_amd_decode_indexed(gpu_ctx.handle, p(sb), sb.size, p(xb), xb.size, p(out), h * w - 1) == -1
    assert lib.nblic_amd_decode_rows(gpu_ctx.handle, p(sb), sb.size, p(xb), xb.size, 3, 9, p(out), 6 * w - 1) == -1
    small = np.zeros(16, np.uint8)
    assert lib.nblic_amd_index_build(gpu_ctx.handle, p(sb), sb.size, 6, p(small), small.size) == len(ix)   # only the size
    assert gpu_ctx.serial_launches() == before, "a refused call launched a kernel"
    assert not out.any()


def test_chain_check_refuses_an_entry_that_does_not_follow(gpu_ctx, pkg, oracle):
    """An entry whose checksums are right but whose rows above are not what the segment before it decodes: each check of
    the entry alone passes, the indexed decode refuses the result."""
    for kind, near, effort in (("n", 0, 1), ("n", 1, 3), ("q", 0, 0)):
        h, w = 30, 100
        s, rec = _stream(oracle, kind, near, effort, h, w, seed=9)
        ix = gpu_ctx.build_index(s, 10)
        head, ents = _split(ix)
        e = bytearray(ents[1])
        rows_at = len(e) - 32 - 2 * w - (24576 if kind == "q" else 0)          # the two rows above the entry (QNBLIC: then its tables)
        e[rows_at + w + 17] ^= 0x01
        forged = _join(head, [ents[0], _reseal_entry(bytes(e))])
        assert pkg.check_index(forged, s)
        with pytest.raises(RuntimeError):
            gpu_ctx.decode_indexed(s, forged)
        assert np.array_equal(gpu_ctx.decode_indexed(s, ix), rec)


def test_wide_rows_and_many_segments(gpu_ctx, pkg, oracle):
    """Rows too wide for the kernels' LDS row ring (taps from memory) and more segments than CUs (the lean decoder)."""
    s, rec = _stream(oracle, "n", 0, 1, 4, 30000, seed=3)
    ix = gpu_ctx.build_index(s, 1)
    assert np.array_equal(gpu_ctx.decode_indexed(s, ix), rec)
    assert np.array_equal(gpu_ctx.decode_rows(s, ix, 2, 3), rec[2:3])
    for kind, near, effort in (("n", 0, 1), ("n", 2, 2), ("q", 0, 0)):
        s, rec = _stream(oracle, kind, near, effort, 300, 40, seed=4)
        ix = gpu_ctx.build_index(s, 1)                          # 300 segments
        assert np.array_equal(gpu_ctx.decode_indexed(s, ix), rec), (kind, near, effort)


def test_faster_than_the_band_decoder(gpu_ctx, pkg):
    """2048 x 1024 SYN-1 -e1 at R = 64: 32 segments side by side against one band decoder."""
    img = inputs.syn1(2048, 1024, 1)
    s = gpu_ctx.encode_batch([img])[0]
    ix = gpu_ctx.build_index(s, 64)
    gpu_ctx.decode_indexed(s, ix)                               # warm up
    t0 = time.perf_counter()
    plane = gpu_ctx.decode_indexed(s, ix)
    t_ix = time.perf_counter() - t0
    t0 = time.perf_counter()
    band = pkg.decompress_bands(s, ctx=gpu_ctx)
    t_band = time.perf_counter() - t0
    assert np.array_equal(plane, img) and np.array_equal(band, img)
    print(f"indexed {t_ix:.3f} s, band decoder {t_band:.3f} s: {t_band / t_ix:.1f}x; index {len(ix)} B, stream {len(s)} B")
    assert t_band >= 8 * t_ix, (t_band, t_ix)


def test_indexed_decode_next_to_encode_batch(gpu_ctx, oracle):
    s, rec = _stream(oracle, "n", 1, 2, 120, 300, seed=12)
    ix = gpu_ctx.build_index(s, 16)
    imgs = [inputs.syn1(64, 96, 40 + k) for k in range(12)]
    want = [oracle.encode(i, 0, 1)[0] for i in imgs]
    got, errs = [], []

    def decode():
        try:
            for _ in range(4):
                got.append(gpu_ctx.decode_indexed(s, ix))
        except Exception as e:                                  # pragma: no cover - reported below
            errs.append(e)

    t = threading.Thread(target=decode)
    t.start()
    for _ in range(4):
        assert gpu_ctx.encode_batch(imgs) == want
    t.join()
    assert not errs, errs
    assert len(got) == 4 and all(np.array_equal(g, rec) for g in got)


def test_integer_redo_on_each_side_of_a_segment_cut(gpu_ctx, pkg, oracle):
    """A 64x64 step edge coded near-lossless at efforts 2 / 3 has pixels that the least squares redo with integers in its
    upper AND its lower 32 rows (CPU harness: 9 + 40 at -n2 -e2, 19 + 3 at -n2 -e3).  With an index entry at row 32 the
    two segments decode side by side to the oracle's plane; each row range decoded on its own counts redone pixels on the
    device (Context.lsq_redo_counts), so the record the second segment starts from carries what the redo needs."""
    img = inputs.make_hard("step_v", 64, 64)
    for near, effort in ((2, 2), (2, 3)):
        s, rec, *_ = oracle.encode(img, near, effort)
        ix = gpu_ctx.build_index(s, 32)
        assert pkg.check_index(ix, s) and len(pkg.index_entries(ix)) == 1
        gpu_ctx.lsq_redo_counts(reset=True)
        assert np.array_equal(gpu_ctx.decode_indexed(s, ix), rec), (near, effort)
        both = gpu_ctx.lsq_redo_counts(reset=True)
        assert np.array_equal(gpu_ctx.decode_rows(s, ix, 0, 32), rec[:32])
        upper = gpu_ctx.lsq_redo_counts(reset=True)
        assert np.array_equal(gpu_ctx.decode_rows(s, ix, 32, 64), rec[32:])
        lower = gpu_ctx.lsq_redo_counts(reset=True)
        print(f"lsq redo on the device: indexed decode step_v 64x64 -n{near} -e{effort}: rows 0..31 {upper}, rows 32..63 {lower}, both segments {both}")
        assert upper[0] >= 1 and lower[0] >= 1 and both[0] == upper[0] + lower[0], (near, effort)
        # the band encoder's own index cuts at the same row
        st = gpu_ctx.stream(img, near, effort, band_rows=20, index_every=32)
        done, whole = st.run()
        own = st.index()
        st.close()
        assert done and whole == s and own == ix


def _c_rows(ctx, s, ix, r0, r1, w, slack=40):
    """nblic_amd_decode_rows through the C entry into a buffer of 0x5A with `slack` bytes behind the range, cap exact:
    (rc, the range's bytes, the slack)."""
    sb, xb = np.frombuffer(s, np.uint8).copy(), np.frombuffer(ix, np.uint8).copy()
    n = (r1 - r0) * w
    out = np.full(n + slack, 0x5A, np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = ctx.lib.nblic_amd_decode_rows(ctx.handle, p(sb), sb.size, p(xb), xb.size, r0, r1, p(out), n)
    return rc, out[:n], out[n:]


def test_row_range_checks_the_boundaries_it_crosses(gpu_ctx, pkg, oracle):
    """Three segments, entry 2 (in front of row 20) forged in its rows above and resealed: a range that crosses that
    boundary is refused and zeroed, nothing behind it touched; a range inside segment 0 and one seeded from the honest
    entry 1 that ends before row 20 decode."""
    h, w = 30, 100
    s, rec = _stream(oracle, "n", 0, 1, h, w, seed=9)
    ix = gpu_ctx.build_index(s, 10)
    head, ents = _split(ix)
    e = bytearray(ents[1])
    e[len(e) - 32 - 2 * w + 150] ^= 0x01
    forged = _join(head, [ents[0], _reseal_entry(bytes(e))])
    assert pkg.check_index(forged, s)
    live = pkg.live_resources()
    rc, rows, slack = _c_rows(gpu_ctx, s, forged, 5, 25, w)
    assert rc == -1 and rows.size == 2000 and not rows.any() and (slack == 0x5A).all()
    assert pkg.live_resources() == live
    for r0, r1 in ((3, 9), (12, 18)):
        rc, rows, slack = _c_rows(gpu_ctx, s, forged, r0, r1, w)
        assert rc == 0 and np.array_equal(rows.reshape(r1 - r0, w), rec[r0:r1]) and (slack == 0x5A).all(), (r0, r1)
        assert pkg.live_resources() == live


@pytest.mark.parametrize("kind,near,effort", [("n", 2, 2), ("q", 0, 0)])
def test_row_range_writes_only_its_bytes(gpu_ctx, pkg, oracle, kind, near, effort):
    """Odd width, unaligned entries, a range over four segments, the unpacked and the packed index: the oracle's rows, and
    the bytes behind them untouched."""
    h, w = 23, 149
    s, rec = _stream(oracle, kind, near, effort, h, w)
    ix = gpu_ctx.build_index(s, 3)
    for x in (ix, pkg.pack_index(ix)):
        rc, rows, slack = _c_rows(gpu_ctx, s, x, 2, 11, w)
        assert rc == 0 and np.array_equal(rows.reshape(9, w), rec[2:11]), (kind, len(x))
        assert (slack == 0x5A).all(), (kind, len(x))
