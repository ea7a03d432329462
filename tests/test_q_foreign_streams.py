"""GPU suite (-m gpu): valid QNBLIC (effort 0) streams that no encoder here writes.  A QNBLIC stream carries its own
twelve frequency tables, and a decoder must take any the format allows; every encoder writes the scaled true counts in the
greedy histogram code, so that is all the decoders had seen.  q_foreign_inputs.py makes streams with other tables -- a
frequency of 1 on every coded symbol (15 bits a pixel, rows of 1.875 w bytes), 128 everywhere (front matter of 3076 words,
the most there can be), tables that put symbol 255 or a far pair under load -- and other codes of the same tables; the
compiled reference decoded every one of them to its plane (tests/golden/make_foreign_q.py, test_q_foreign_host.py, which
also asserts what the set reaches).  QNBLIC is lossless: here every decoder on the GPU -- batch, into device memory,
drop-in, band decoder fed every which way and across checkpoints, seek index built, packed, unpacked on the device and
decoded through -- must give the plane the stream was made from, bit for bit, case by case."""
import ctypes as C
import hashlib
import struct
import time

import numpy as np
import pytest

import q_foreign_inputs as qf

pytestmark = pytest.mark.gpu

CKPT_HEAD = "<8sI8i"          # "NBLDCKPT", version, kind, h, w, near, k_step, effort, band_rows, next_row
CKPT_HEAD_BYTES = 168         # a checkpoint's body starts here with the state record: next_row, status (int32), pos (uint64), lo = the rANS state (uint32)
Q_RECORD_BYTES = 12352        # the state record of a QNBLIC entry; the two rows above follow it


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _is_wide(c):
    return c.plane.shape[1] >= qf.WIDE_CACHED


def _pick(oracle, keys):
    return [qf.case_of(oracle, *k) for k in keys]


def _tag(c):
    return (c.plane_name, c.family, c.policy)


# ---- 1. batch decoders ---------------------------------------------------------------------------------------------
def test_batch_every_stream_in_one_call(gpu_ctx, pkg, oracle):
    """All streams in one decode_batch.  The widest plane's rows do not fit in LDS next to the decoder's tables: its jobs
    take their taps from memory, the others (the kernel compares per job) from the row ring."""
    cs = qf.cases(oracle)
    assert pkg.serial_plan(True, 0, len(cs), max(c.plane.shape[1] for c in cs)) == 0
    assert pkg.serial_plan(True, 0, 1, qf.WIDE_UNCACHED) == 0 and pkg.serial_plan(True, 0, 1, qf.WIDE_CACHED) == pkg.PLAN_ROWS_IN_LDS
    assert pkg.serial_plan(True, 0, len(cs), qf.WIDE_CACHED) == pkg.PLAN_ROWS_IN_LDS          # one LDS image, however many streams
    assert sum(c.plane.shape[1] == qf.WIDE_UNCACHED for c in cs) >= 8 and sum(c.plane.shape[1] == qf.WIDE_CACHED for c in cs) >= 8
    t0 = time.perf_counter()
    got = gpu_ctx.decode_batch([c.stream for c in cs])
    print(f"decode_batch: {len(cs)} streams, {sum(len(c.stream) for c in cs)} bytes, {time.perf_counter() - t0:.3f} s")
    assert len(got) == len(cs)
    for g, c in zip(got, cs):
        assert g is not None, _tag(c)
        assert np.array_equal(g[0], c.plane) and g[1:] == (0, 0), _tag(c)
    stored = qf.golden()
    groups = {}
    for g, c in zip(got, cs):
        groups.setdefault(f"{c.plane_name}/{c.family}", []).append(g[0].tobytes())
    for key, planes in groups.items():
        assert sha(b"".join(planes)) == stored[key]["planes_sha256"], key


def test_batch_one_class_of_more_than_256_images(gpu_ctx, pkg, oracle):
    """The streams of the small planes twice over: 528 images of one launch, every one with its rows in LDS."""
    cs = [c for c in qf.cases(oracle) if not _is_wide(c)] * 2
    assert len(cs) > 256
    assert pkg.serial_plan(True, 0, len(cs), max(c.plane.shape[1] for c in cs)) == pkg.PLAN_ROWS_IN_LDS
    t0 = time.perf_counter()
    got = gpu_ctx.decode_batch([c.stream for c in cs])
    print(f"decode_batch: {len(cs)} streams of the small planes, {time.perf_counter() - t0:.3f} s")
    for g, c in zip(got, cs):
        assert g is not None and np.array_equal(g[0], c.plane), _tag(c)


def test_decode_batch_into_a_device_tensor(gpu_ctx, pkg, oracle):
    """Every stream of the small planes in one decode_batch_into, uint8: each plane in its window of one tensor, the rest
    of the tensor untouched."""
    import torch
    cs = [c for c in qf.cases(oracle) if not _is_wide(c)]
    hm, wm = max(c.plane.shape[0] for c in cs), max(c.plane.shape[1] for c in cs)
    out = torch.full((len(cs), hm + 1, wm + 3), 0xA7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    status = gpu_ctx.decode_batch_into([c.stream for c in cs], [out[k, :c.plane.shape[0], :c.plane.shape[1]] for k, c in enumerate(cs)])
    print(f"decode_batch_into: {len(cs)} streams, {time.perf_counter() - t0:.3f} s")
    assert status == [0] * len(cs)
    got = out.cpu().numpy()
    for k, c in enumerate(cs):
        h, w = c.plane.shape
        assert np.array_equal(got[k, :h, :w], c.plane), _tag(c)
        assert (got[k, h:] == 0xA7).all() and (got[k, :, w:] == 0xA7).all(), _tag(c)


# ---- 2. drop-in QNBLICdecompress ---------------------------------------------------------------------------------------
DROPIN = [("noise_17x13", "uniform", "greedy"), ("noise_17x13", "ones_on_255", "plain"), ("syn1_64x64", "ones_on_128", "greedy"),
          ("syn1_64x64", "uniform", "widest"), ("spikes_32x48", "sparse", "runs"), ("checker_33x70", "rotated", "runs"),
          ("flat_8x8", "far_pair", "greedy"), ("flat_8x8", "far_pair_mirror", "plain"), ("noise_1x1", "uniform", "greedy"),
          ("noise_1x300", "ones_on_0", "widest"), ("syn1_2x256", "smoothed", "plain"), (f"syn1_3x{qf.WIDE_CACHED}", "ones_on_254", "greedy")]


def test_dropin_decompress(gpu_ctx, pkg, oracle):               # gpu_ctx first: torch must initialise HIP before the library does
    """The drop-in decoder is handed a pointer and no length: it fetches the stream in steps.  In steps of 4096 bytes the
    tables of a 3076-word front matter are complete only with the second step."""
    from oracle.oracle import out_capacity
    lib = pkg.load_library()
    cs = _pick(oracle, DROPIN)
    assert any(qf.tables_of(c.stream)[1] == qf.MAX_FRONT_WORDS for c in cs)
    assert any(len(c.stream) > out_capacity(*c.plane.shape) for c in cs)
    t0 = time.perf_counter()
    for chunk in (0, 4096):                                              # 0: the default step
        pkg.set_default_feed_chunk(chunk)
        try:
            for c in cs:
                d = pkg.qdecompress(c.stream)
                assert d is not None and np.array_equal(d, c.plane), _tag(c) + (chunk,)
                buf = np.frombuffer(c.stream, np.uint8).copy().view(np.uint16)
                img = np.full(c.plane.shape, 0x5A, np.uint8)
                hh, ww = C.c_int(), C.c_int()
                rc = lib.QNBLICdecompress(buf.ctypes.data_as(C.POINTER(C.c_uint16)), img.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(hh), C.byref(ww))
                assert rc == 0 and (hh.value, ww.value) == c.plane.shape and np.array_equal(img, c.plane), _tag(c) + (chunk,)
        finally:
            pkg.set_default_feed_chunk(0)
    print(f"drop-in: {4 * len(cs)} decodes in {time.perf_counter() - t0:.3f} s")


# ---- 3. band decoder ---------------------------------------------------------------------------------------------------
BAND = [("syn1_64x64", "ones_on_128", "greedy"), ("syn1_64x64", "uniform", "plain"), ("syn1_64x64", "sparse", "widest"),
        ("checker_33x70", "sparse", "runs"), ("checker_33x70", "uniform", "greedy"), ("checker_33x70", "ones_on_255", "plain"),
        ("spikes_32x48", "rotated", "widest"), ("spikes_32x48", "ones_on_254", "runs"), ("noise_17x13", "uniform", "greedy"),
        ("noise_17x13", "ones_on_0", "plain"), ("flat_8x8", "far_pair", "greedy"), ("flat_8x8", "far_pair_mirror", "runs"),
        ("noise_1x300", "ones_on_0", "runs"), ("syn1_2x256", "smoothed", "widest"), ("syn1_2x256", "ones_on_128", "plain"),
        ("noise_1x1", "uniform", "greedy"), ("noise_1x1", "sparse", "plain")]
BAND_WIDE = [(f"syn1_3x{qf.WIDE_CACHED}", "ones_on_254", "greedy"), (f"syn1_3x{qf.WIDE_UNCACHED}", "ones_on_128", "plain"),
             (f"syn1_3x{qf.WIDE_UNCACHED}", "uniform", "greedy")]


def _band_decode(ctx, stream, band_rows, pieces):
    """The stream through one band decoder, the next of `pieces` (byte counts; the last one repeats) fed whenever it
    asks for input, `final` with the last byte alone.  Returns (plane, progress, pieces fed)."""
    d = ctx.decoder(band_rows)
    parts, at, feeds = [], 0, 0
    pieces = iter(pieces)
    n = 1
    try:
        for _ in range(1_000_000):
            rc, rows, first = d.run(max_rows=band_rows)
            assert first == sum(p.shape[0] for p in parts)
            if rows.size:
                parts.append(rows)
            if rc == 1:
                break
            if rc == 2:
                assert at < len(stream), "the decoder asks for more than the stream"
                n = next(pieces, n)
                d.feed(stream[at:at + n], final=at + n >= len(stream))
                at += n
                feeds += 1
        prog = d.progress()
    finally:
        d.close()
    return np.concatenate(parts), prog, feeds


def _check_band(c, got, prog, what):
    assert np.array_equal(got, c.plane), _tag(c) + what
    assert prog["state"] == 1 and prog["rows_done"] == c.plane.shape[0] and prog["sha256"] == sha(c.plane.tobytes()), _tag(c) + what


def test_band_decoder_pieces_of_two_bytes_per_pixel_of_a_row(gpu_ctx, pkg, oracle):
    """Pieces of exactly 2 w bytes: fewer than a launch wants in front of a row (2 w + 8), so a decoder that is not final
    starves in front of every row it has not two pieces for, and rows of 1.875 w bytes leave it little to spare.  The last
    row is never begun before the stream is final, so the decoder asks for every piece."""
    t0 = time.perf_counter()
    cs = _pick(oracle, BAND + BAND_WIDE)
    for c in cs:
        w = c.plane.shape[1]
        for br in (1, 5):
            if _is_wide(c) and br == 5:
                continue
            got, prog, feeds = _band_decode(gpu_ctx, c.stream, br, [2 * w])
            _check_band(c, got, prog, ("2w", br))
            assert feeds == -(-len(c.stream) // (2 * w)), _tag(c) + (br, feeds)                 # it asked until the last byte was in
    print(f"band decoder, pieces of 2 w bytes: {len(cs)} streams in {time.perf_counter() - t0:.3f} s")


def test_band_decoder_first_piece_ends_where_the_first_launch_has_just_enough(gpu_ctx, pkg, oracle):
    """The first piece ends 2 w + 8 + k bytes behind the tables, k = 0 .. 13: around what the first launch asks for, which
    has the four bytes of the rANS state to read before row 0 as well.  (With k < 4 a launch used to read the state,
    starve in front of row 0 and leave the next launch to read the state again, four bytes further on.)  Native streams
    too: the piece size alone decides."""
    import inputs
    native = [qf.Case(name, "native", "greedy", img, None, oracle.qencode(img))
              for name, img in (("syn1_23x150", inputs.syn1(23, 150, 5)), ("noise_17x13", inputs.noise(17, 13)))]
    cs = native + _pick(oracle, [("checker_33x70", "uniform", "greedy"), ("syn1_64x64", "ones_on_128", "greedy"), ("noise_17x13", "uniform", "plain"),
                                 ("spikes_32x48", "sparse", "runs")])
    t0 = time.perf_counter()
    for c in cs:
        w = c.plane.shape[1]
        first = 2 * qf.tables_of(c.stream)[1] + 2 * w + 8
        assert first + 13 < len(c.stream), _tag(c)
        for k in range(14):
            for br in (1, 4):
                got, prog, feeds = _band_decode(gpu_ctx, c.stream, br, [first + k, 1 << 30])
                _check_band(c, got, prog, ("first piece", k, br))
                assert feeds == 2, _tag(c) + (k, br)
    print(f"band decoder, first piece at the first launch's need: {len(cs)} streams x 14 x 2 in {time.perf_counter() - t0:.3f} s")


def test_band_decoder_random_pieces(gpu_ctx, pkg, oracle):
    rng = np.random.default_rng(20250)
    t0 = time.perf_counter()
    cs = _pick(oracle, BAND)
    for c in cs:
        for br in (1, 3):
            got, prog, _ = _band_decode(gpu_ctx, c.stream, br, (int(v) for v in rng.integers(1, 700, 100000)))
            _check_band(c, got, prog, ("random", br))
    print(f"band decoder, random pieces: {len(cs)} streams in {time.perf_counter() - t0:.3f} s")


def test_band_decoder_tables_that_complete_late(gpu_ctx, pkg, oracle):
    """The first 6152 bytes -- the longest front matter there is -- in pieces of 40, the rest at once.  A QNBLIC stream is
    described only when its tables are complete: for a uniform stream with the last of the 154 pieces, not before."""
    t0 = time.perf_counter()
    cs = [c for c in _pick(oracle, BAND) if c.family == "uniform"] + _pick(oracle, [("syn1_64x64", "smoothed", "plain"), ("spikes_32x48", "uniform", "runs")])
    assert len(cs) >= 5
    for c in cs:
        front = 2 * qf.tables_of(c.stream)[1]
        assert len(c.stream) > 6152 and (front == 6152 or c.family != "uniform"), _tag(c)
        d = gpu_ctx.decoder(4)
        try:
            at, parts = 0, []
            while at < 6152:
                n = min(40, 6152 - at)
                d.feed(c.stream[at:at + n])
                at += n
                rc, rows, _ = d.run(max_rows=4)
                if at < front:
                    assert rc == 2 and rows.size == 0 and d.info() is None, _tag(c) + (at,)
                else:
                    assert d.info() == {"kind": "QNBLIC", "height": c.plane.shape[0], "width": c.plane.shape[1], "near": 0, "effort": 0}, _tag(c) + (at,)
                    parts += [rows] if rows.size else []
            d.feed(c.stream[at:], final=True)
            while True:
                rc, rows, first = d.run(max_rows=4)
                assert rc in (0, 1) and first == sum(p.shape[0] for p in parts), _tag(c)
                parts.append(rows)
                if rc == 1:
                    break
            _check_band(c, np.concatenate(parts), d.progress(), ("late tables",))
        finally:
            d.close()
    print(f"band decoder, late tables: {len(cs)} streams in {time.perf_counter() - t0:.3f} s")


def test_band_decoder_checkpoint_after_every_band(gpu_ctx, pkg, oracle):
    """The maximum-rate stream and the uniform stream of two planes: a checkpoint after every band of 4 rows, each resumed
    on a second context and fed from the offset it names."""
    cs = _pick(oracle, [("checker_33x70", "ones_on_128", "greedy"), ("checker_33x70", "uniform", "plain"),
                        ("spikes_32x48", "ones_on_254", "runs"), ("spikes_32x48", "uniform", "greedy")])
    ctx2 = pkg.Context(device=0, n_slots=1, n_coders=1)
    t0 = time.perf_counter()
    n_ck = 0
    try:
        for c in cs:
            h, w = c.plane.shape
            br = 4
            d = gpu_ctx.decoder(br)
            d.feed(c.stream, final=True)
            done = []
            while True:
                rc, rows, first = d.run(max_rows=br)
                done.append(rows)
                if rc == 1:
                    break
                assert rc == 0, _tag(c)
                ck, prog = d.checkpoint(), d.progress()
                head = struct.unpack_from(CKPT_HEAD, ck)
                assert head[0] == b"NBLDCKPT" and head[2:] == (1, h, w, 0, 3, 0, br, prog["rows_done"]), _tag(c)
                assert gpu_ctx.check_decoder_checkpoint(ck), _tag(c)
                r = ctx2.decoder(checkpoint=ck)
                r.feed(c.stream[prog["feed_from"]:], final=True)
                rc2, rest, first2 = r.run()
                assert rc2 == 1 and first2 == prog["rows_done"], _tag(c)
                assert np.array_equal(np.concatenate(done + [rest]), c.plane), _tag(c) + (first2,)
                assert r.progress()["sha256"] == sha(c.plane.tobytes()), _tag(c) + (first2,)
                r.close()
                n_ck += 1
            d.close()
            assert np.array_equal(np.concatenate(done), c.plane), _tag(c)
    finally:
        ctx2.close()
    print(f"band decoder: {n_ck} checkpoints of {len(cs)} streams resumed in {time.perf_counter() - t0:.3f} s")


# ---- 4. seek index -----------------------------------------------------------------------------------------------------
INDEXED = [("syn1_64x64", f, p, 16) for f, p in (("ones_on_128", "greedy"), ("uniform", "plain"), ("sparse", "runs"), ("rotated", "widest"), ("ones_on_255", "runs"))] + \
          [("checker_33x70", f, p, 8) for f, p in (("ones_on_254", "plain"), ("uniform", "greedy"), ("sparse", "widest"), ("smoothed", "runs"), ("ones_on_0", "greedy"))] + \
          [("spikes_32x48", "rotated", "runs", 8), ("spikes_32x48", "uniform", "widest", 5), ("noise_17x13", "ones_on_255", "greedy", 4), ("noise_17x13", "uniform", "plain", 3)]
_INDEX = {}


def _indexed(gpu_ctx, oracle):
    """[(case, every_rows, index)], the indexes from the serial builder, once for the module."""
    if "ix" not in _INDEX:
        t0 = time.perf_counter()
        _INDEX["ix"] = [(qf.case_of(oracle, name, fam, pol), r, gpu_ctx.build_index(qf.case_of(oracle, name, fam, pol).stream, r)) for name, fam, pol, r in INDEXED]
        print(f"build_index: {len(INDEXED)} streams in {time.perf_counter() - t0:.3f} s")
    return _INDEX["ix"]


def test_index_entries_name_the_coder_of_the_host_entropy_stage(gpu_ctx, pkg, oracle):
    """Every entry's rANS state and stream position against pkg.q_entropy_entries(level | symbol << 8, entry rows, hist=T),
    which reports the coder in front of a row as (state, words emitted from the end of the pass down to that row): the
    decoder there has read all of the stream but those words (test_qindexed_batch_host.py decode_from)."""
    for c, every, ix in _indexed(gpu_ctx, oracle):
        plane, qd, y, _ = qf.models(oracle)[c.plane_name]
        h, w = plane.shape
        count = (h - 1) // every
        assert count >= 3, _tag(c)
        assert struct.unpack_from("<8i", ix, 12) == (1, h, w, 0, 3, 0, every, count), _tag(c)
        assert pkg.check_index(ix, c.stream) and pkg.check_index(ix, c.stream, gpu_ctx), _tag(c)
        rows = [every * (k + 1) for k in range(count)]
        words = (qd.astype(np.uint16) | (y.astype(np.uint16) << 8)).reshape(h, w)
        _, want = pkg.q_entropy_entries(words, rows, hist=c.tables)
        entries = pkg.index_entries(ix)
        assert len(entries) == count == len(want)
        for e, r, (state, emitted) in zip(entries, rows, want):
            head = struct.unpack_from(CKPT_HEAD, e)
            assert head[2:] == (1, h, w, 0, 3, 0, every, r), _tag(c) + (r,)
            next_row, status, pos, lo = struct.unpack_from("<iiQI", e, CKPT_HEAD_BYTES)
            assert (next_row, status) == (r, 0), _tag(c) + (r,)
            assert lo == state, _tag(c) + (r, lo, state)
            assert pos == len(c.stream) - 2 * emitted, _tag(c) + (r, pos, emitted)
            rows_above = np.frombuffer(e, np.uint8, 2 * w, CKPT_HEAD_BYTES + Q_RECORD_BYTES).reshape(2, w)
            assert np.array_equal(rows_above, plane[r - 2:r]), _tag(c) + (r,)


def test_index_build_batch_is_the_serial_builders(gpu_ctx, pkg, oracle):
    made = _indexed(gpu_ctx, oracle)
    t0 = time.perf_counter()
    got, planes = gpu_ctx.build_index_batch([c.stream for c, _, _ in made], [r for _, r, _ in made], planes=True)
    print(f"build_index_batch: {len(made)} streams in {time.perf_counter() - t0:.3f} s")
    for g, p, (c, every, ix) in zip(got, planes, made):
        assert g == ix, _tag(c)
        assert p is not None and np.array_equal(p, c.plane), _tag(c)


def test_decodes_through_the_index(gpu_ctx, pkg, oracle):
    made = _indexed(gpu_ctx, oracle)
    t0 = time.perf_counter()
    windows = []
    for k, (c, every, ix) in enumerate(made):
        h = c.plane.shape[0]
        assert np.array_equal(gpu_ctx.decode_indexed(c.stream, ix), c.plane), _tag(c)
        for r0, r1 in ((every - 1, every + 1), (every + 1, 2 * every + 2), (2 * every, h), (1, 2)):
            assert np.array_equal(gpu_ctx.decode_rows(c.stream, ix, r0, r1), c.plane[r0:r1]), _tag(c) + (r0, r1)
        windows.append(((k * 3) % (h - 2), min(h, (k * 3) % (h - 2) + 2 + every)))
    pairs = [(c.stream, ix) for c, _, ix in made]
    for g, (c, _, _) in zip(gpu_ctx.decode_batch_indexed(pairs), made):
        assert g is not None and np.array_equal(g, c.plane), _tag(c)
    for g, (c, _, _), (r0, r1) in zip(gpu_ctx.decode_batch_indexed(pairs, rows=windows), made, windows):
        assert g is not None and np.array_equal(g, c.plane[r0:r1]), _tag(c) + (r0, r1)
    print(f"decodes through the index: {len(made)} streams in {time.perf_counter() - t0:.3f} s")


def test_packed_index_unpacks_on_the_device_to_the_unpacked_one(gpu_ctx, pkg, oracle):
    made = _indexed(gpu_ctx, oracle)
    t0 = time.perf_counter()
    packed = [pkg.pack_index(ix) for _, _, ix in made]
    for (c, every, ix), px in zip(made, packed):
        w = c.plane.shape[1]
        assert pkg.index_is_packed(px) and pkg.unpack_index(px) == ix and pkg.check_index(px, c.stream), _tag(c)
        count = struct.unpack_from("<i", ix, 40)[0]
        eb = (len(ix) - 96 - 32) // count
        tab = Q_RECORD_BYTES + 2 * w                                       # what of a body the device holds: all but the tables
        (bodies, guard), = gpu_ctx.debug_index_unpack([(px, 3, count, 0)])
        assert (guard == 0xA7).all(), _tag(c)
        for e in range(count):
            at = 96 + e * eb + 8 + CKPT_HEAD_BYTES
            assert bodies[e, :tab].tobytes() == ix[at:at + tab], _tag(c) + (e,)
        assert np.array_equal(gpu_ctx.decode_indexed(c.stream, px), c.plane), _tag(c)
        assert np.array_equal(gpu_ctx.decode_rows(c.stream, px, every + 1, 2 * every + 1), c.plane[every + 1:2 * every + 1]), _tag(c)
    mixed = [(c.stream, px if k % 2 else ix) for k, ((c, _, ix), px) in enumerate(zip(made, packed))]
    for g, (c, _, _) in zip(gpu_ctx.decode_batch_indexed(mixed), made):
        assert g is not None and np.array_equal(g, c.plane), _tag(c)
    print(f"packed indexes: {len(made)} streams in {time.perf_counter() - t0:.3f} s")
