"""GPU suite (-m gpu): valid streams that no encoder here writes.  A decoder takes k_step from byte 14 of the header and
accepts any 3..16 with any near 0..9 (NBLIC.c:733-745, :765); every encoder writes clip(3 + 2 near, 3, 16), so only eight
of the 140 pairs ever reached a kernel.  The oracle codes small planes with all 140 pairs (Oracle.encode(k_step=)); the
compiled reference decoded every one of those streams to the oracle's reconstruction (tests/golden/make_foreign.py,
test_oracle.py).  Here every decoder on the GPU -- batch (full and lean image), drop-in, band decoder across a checkpoint,
seek index, rows in LDS and not -- must give the oracle's plane bit for bit, per case, and in aggregate the planes whose
hashes the reference left in tests/golden/foreign_streams.json.

Which regimes of decode_symbol the streams reach (inside the lanes, beyond the lanes in the same tree, escalation to the
next level's tree) is asserted on the CPU: test_oracle.py test_foreign_planes_reach_every_walk_regime."""
import ctypes as C
import hashlib
import struct
import time

import numpy as np
import pytest

import inputs

pytestmark = pytest.mark.gpu


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


_CACHE = {}


def _all(oracle):
    """name -> [((near, k_step, effort), stream, reconstruction)] x 420, efforts outermost: coded once for the module."""
    if "all" not in _CACHE:
        t0 = time.perf_counter()
        _CACHE["all"] = {name: inputs.foreign_streams(oracle, plane) for name, plane in inputs.foreign_planes().items()}
        print(f"oracle: {sum(len(v) for v in _CACHE['all'].values())} foreign streams coded in {time.perf_counter() - t0:.1f} s")
    return _CACHE["all"]


def _check(got, cases, tag):
    """Each decode_batch result against the oracle's plane and the header's (near, effort)."""
    assert len(got) == len(cases)
    for g, ((near, k_step, effort), s, rec) in zip(got, cases):
        case = (tag, near, k_step, effort)
        assert g is not None, case
        assert np.array_equal(g[0], rec), case
        assert (g[1], g[2]) == (near, effort), case


# ---- 1. batch decoders ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kodak05", "blocks", "noise", "syn1", "spikes", "checker"])
def test_batch_every_header_of_a_plane_full_image(gpu_ctx, pkg, oracle, name):
    """All 420 (near, k_step, effort) streams of one plane in one decode_batch: three effort classes of 140 images, each
    at most 256 and so the full LDS image.  Per case the oracle's plane; per effort the hash of the planes the reference
    decoded the same streams to."""
    cases = _all(oracle)[name]
    w = cases[0][2].shape[1]
    for effort in inputs.FOREIGN_EFFORTS:
        assert pkg.serial_plan(True, effort, 140, w) == pkg.PLAN_ROWS_IN_LDS          # not lean, rows cached
    t0 = time.perf_counter()
    got = gpu_ctx.decode_batch([c[1] for c in cases])
    print(f"decode_batch {name}: 420 streams, full image, {time.perf_counter() - t0:.3f} s")
    _check(got, cases, name)
    stored = inputs.foreign_golden()
    for k, effort in enumerate(inputs.FOREIGN_EFFORTS):
        part = slice(140 * k, 140 * (k + 1))
        assert [c[0] for c in cases[part]] == [(n, ks, effort) for n, ks in inputs.FOREIGN_PAIRS]
        want = stored[f"{name}_e{effort}"]
        assert sha(b"".join(c[1] for c in cases[part])) == want["streams_sha256"], (name, effort)
        assert sha(b"".join(g[0].tobytes() for g in got[part])) == want["planes_sha256"], (name, effort)


@pytest.mark.parametrize("effort", inputs.FOREIGN_EFFORTS)
def test_batch_every_plane_of_an_effort_lean_image(gpu_ctx, pkg, oracle, effort):
    """The 840 streams of one effort, every plane and header together: one class of more than 256 images, the lean image."""
    cases, tags = [], []
    for name, cs in _all(oracle).items():
        for c in cs:
            if c[0][2] == effort:
                cases.append(c)
                tags.append(name)
    assert len(cases) == 840
    max_w = max(c[2].shape[1] for c in cases)
    assert pkg.serial_plan(True, effort, len(cases), max_w) == pkg.PLAN_LEAN | pkg.PLAN_ROWS_IN_LDS
    t0 = time.perf_counter()
    got = gpu_ctx.decode_batch([c[1] for c in cases])
    print(f"decode_batch effort {effort}: 840 streams, lean image, {time.perf_counter() - t0:.3f} s")
    for g, c, tag in zip(got, cases, tags):
        _check([g], [c], tag)
    stored = inputs.foreign_golden()
    at = 0
    for name in _all(oracle):
        assert sha(b"".join(g[0].tobytes() for g in got[at:at + 140])) == stored[f"{name}_e{effort}"]["planes_sha256"], (name, effort)
        at += 140


def test_batch_few_effort3_streams(gpu_ctx, pkg, oracle):
    """At most 64 effort-3 streams in one call, lossless, the unpaired steps first.  (A batch this small gives an
    ENCODE of effort 3 two waves per image; the decoders have one kernel per effort and image size class, asserted here.)"""
    steps = (4, 6, 8, 10, 12, 14, 16, 5, 15, 3)
    cases, tags = [], []
    for name, cs in _all(oracle).items():
        for c in cs:
            if c[0][2] == 3 and c[0][0] == 0 and c[0][1] in steps:
                cases.append(c)
                tags.append(name)
    assert len(cases) == 60
    assert pkg.serial_plan(False, 3, len(cases), 81) & pkg.PLAN_TWO_WAVES
    assert pkg.serial_plan(True, 3, len(cases), 81) == pkg.PLAN_ROWS_IN_LDS
    got = gpu_ctx.decode_batch([c[1] for c in cases])
    for g, c, tag in zip(got, cases, tags):
        _check([g], [c], tag)


# ---- 2. drop-in NBLICdecompress ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kodak05", "spikes"])
def test_dropin_decompress_every_step(gpu_ctx, pkg, oracle, name):      # gpu_ctx first: torch must initialise HIP before the library does
    lib = pkg.load_library()
    u8p = C.POINTER(C.c_uint8)
    n = 0
    t0 = time.perf_counter()
    for (near, k_step, effort), s, rec in _all(oracle)[name]:
        if near not in (0, 1, 9):
            continue
        case = (name, near, k_step, effort)
        d = pkg.decompress(s)
        assert d is not None and np.array_equal(d[0], rec) and d[1:] == (near, effort), case
        buf = np.frombuffer(s, np.uint8).copy()
        img = np.full(rec.shape, 0x5A, np.uint8)
        hh, ww, nn, ee = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        rc = lib.NBLICdecompress(0, buf.ctypes.data_as(u8p), img.ctypes.data_as(u8p), C.byref(hh), C.byref(ww), C.byref(nn), C.byref(ee))
        assert rc == 0 and (hh.value, ww.value, nn.value, ee.value) == rec.shape + (near, effort), case
        assert np.array_equal(img, rec), case
        n += 1
    assert n == 14 * 3 * 3
    print(f"drop-in {name}: {2 * n} decodes in {time.perf_counter() - t0:.3f} s")


# ---- 3. / 4. band decoder and seek index ---------------------------------------------------------------------------
BAND_PAIRS = [(0, 16), (0, 8), (1, 12), (9, 3), (2, 4), (0, 6)]
BAND_EFFORTS = (1, 3)
CKPT_HEAD = "<8sI8i"          # "NBLDCKPT", version, kind, h, w, near, k_step, effort, band_rows, next_row


def _band_planes():
    _, arrays = inputs.fixtures()
    return {"kodak05_64x96": np.ascontiguousarray(arrays["kodak_crops"][4]), "spikes_80x48": inputs.spikes(80, 48)}


def _band_cases(oracle):
    """[(tag, plane, (near, k_step, effort), stream, reconstruction)]: 2 planes x 6 pairs x 2 efforts, coded once."""
    if "band" not in _CACHE:
        out = []
        for tag, plane in _band_planes().items():
            for c in inputs.foreign_streams(oracle, plane, BAND_EFFORTS, BAND_PAIRS):
                out.append((tag, plane) + c)
        _CACHE["band"] = out
    return _CACHE["band"]


def _fed_in_pieces(ctx, stream, band_rows, rng):
    d = ctx.decoder(band_rows)
    parts, at = [], 0
    try:
        for _ in range(100000):
            rc, rows, first = d.run(max_rows=band_rows)
            assert first == sum(p.shape[0] for p in parts)
            if rows.size:
                parts.append(rows)
            if rc == 1:
                break
            if rc == 2:
                n = int(rng.integers(1, 700))
                d.feed(stream[at:at + n], final=at + n >= len(stream))
                at += n
        prog = d.progress()
    finally:
        d.close()
    return np.concatenate(parts), prog


def test_band_decoder_random_pieces_and_a_checkpoint(gpu_ctx, pkg, oracle):
    """Bands of 1 and 5 rows, the stream fed in seeded random pieces; then a checkpoint after the first band, whose head
    names the stream's k_step, resumed on a second context: the oracle's rows and their running SHA-256."""
    rng = np.random.default_rng(4321)
    ctx2 = pkg.Context(device=0, n_slots=1, n_coders=1)
    t0 = time.perf_counter()
    try:
        for tag, plane, (near, k_step, effort), s, rec in _band_cases(oracle):
            for br in (1, 5):
                case = (tag, near, k_step, effort, br)
                got, prog = _fed_in_pieces(gpu_ctx, s, br, rng)
                assert np.array_equal(got, rec), case
                assert prog["state"] == 1 and prog["rows_done"] == rec.shape[0] and prog["sha256"] == sha(rec.tobytes()), case
                d = gpu_ctx.decoder(br)
                d.feed(s, final=True)
                assert d.info() == {"kind": "NBLIC", "height": rec.shape[0], "width": rec.shape[1], "near": near, "effort": effort}, case
                rc, rows, first = d.run(max_rows=br)
                assert rc == 0 and first == 0 and rows.shape[0] == br, case
                ck, ff = d.checkpoint(), d.progress()["feed_from"]
                d.close()
                head = struct.unpack_from(CKPT_HEAD, ck)
                assert head[0] == b"NBLDCKPT" and head[2:] == (0, rec.shape[0], rec.shape[1], near, k_step, effort, br, br), case
                assert gpu_ctx.check_decoder_checkpoint(ck), case
                r = ctx2.decoder(checkpoint=ck)
                r.feed(s[ff:], final=True)
                rc, rest, first = r.run()
                assert rc == 1 and first == br and np.array_equal(np.concatenate([rows, rest]), rec), case
                assert r.progress()["sha256"] == sha(rec.tobytes()), case
                r.close()
    finally:
        ctx2.close()
    print(f"band decoder: {len(_band_cases(oracle))} streams x bands of 1 and 5 rows in {time.perf_counter() - t0:.3f} s")


def test_seek_index_names_the_step(gpu_ctx, pkg, oracle):
    """build_index(R = 16) of every band-test stream: the index is the index of ITS stream, not of the same plane coded
    with the encoders' own k_step for that near (nor of that stream with only the header's step changed); the indexed decode
    and row ranges across an entry give the oracle's rows."""
    t0 = time.perf_counter()
    for tag, plane, (near, k_step, effort), s, rec in _band_cases(oracle):
        case = (tag, near, k_step, effort)
        h = rec.shape[0]
        ix = gpu_ctx.build_index(s, 16)
        assert struct.unpack_from("<8i", ix, 12) == (0, h, rec.shape[1], near, k_step, effort, 16, (h - 1) // 16), case
        assert pkg.check_index(ix, s) and pkg.check_index(ix, s, gpu_ctx), case
        for e in pkg.index_entries(ix):
            assert struct.unpack_from(CKPT_HEAD, e)[6] == k_step, case
        paired = inputs.paired_k_step(near)
        assert paired != k_step
        other = oracle.encode(plane, near, effort)[0]
        assert other[14] == paired and other[:14] == s[:14] and other[15] == s[15]
        assert not pkg.check_index(ix, other), case
        assert not pkg.check_index(ix, s[:14] + bytes([paired]) + s[15:]), case
        before = gpu_ctx.serial_launches()
        with pytest.raises(RuntimeError):
            gpu_ctx.decode_indexed(other, ix)
        assert gpu_ctx.serial_launches() == before, case
        assert np.array_equal(gpu_ctx.decode_indexed(s, ix), rec), case
        for r0, r1 in ((10, 40), (15, 17), (31, 33), (16, h)):
            assert np.array_equal(gpu_ctx.decode_rows(s, ix, r0, r1), rec[r0:r1]), case + (r0, r1)
    print(f"seek index: {len(_band_cases(oracle))} streams in {time.perf_counter() - t0:.3f} s")


# ---- 5. rows too wide for the LDS row ring -------------------------------------------------------------------------
def test_wide_rows_take_the_uncached_taps(gpu_ctx, pkg, oracle):
    from oracle.oracle import syn1
    img = syn1(2, 30000, 6)
    rng = np.random.default_rng(5)
    for near, k_step, effort in ((0, 16, 1), (1, 12, 3)):
        case = (near, k_step, effort)
        assert pkg.serial_plan(True, effort, 1, 30000) == 0 and pkg.serial_plan(True, effort, 1, 30000, False) == 0     # not lean, taps from memory
        assert pkg.serial_plan(True, effort, 1, 20000) == pkg.PLAN_ROWS_IN_LDS
        s, rec, *_ = oracle.encode(img, near, effort, k_step=k_step)
        assert s[14] == k_step
        t0 = time.perf_counter()
        g = gpu_ctx.decode_batch([s])[0]
        t1 = time.perf_counter()
        assert g is not None and np.array_equal(g[0], rec) and g[1:] == (near, effort), case
        d = gpu_ctx.decoder(1)
        at, parts = 0, []
        while True:
            rc, rows, _ = d.run(max_rows=1)
            if rows.size:
                parts.append(rows)
            if rc == 1:
                break
            if rc == 2:
                n = int(rng.integers(1, 20000))
                d.feed(s[at:at + n], final=at + n >= len(s))
                at += n
        digest = d.progress()["sha256"]
        d.close()
        assert np.array_equal(np.concatenate(parts), rec) and digest == sha(rec.tobytes()), case
        print(f"2 x 30000 -n{near} k_step {k_step} -e{effort}: decode_batch {t1 - t0:.3f} s, band decoder {time.perf_counter() - t1:.3f} s")


# ---- 6. refusals ---------------------------------------------------------------------------------------------------
def test_steps_outside_3_to_16_are_refused_before_any_launch(gpu_ctx, pkg, oracle):
    plane = inputs.spikes()
    ix_of = {}
    for near, k_step in ((0, 8), (9, 16)):
        s = oracle.encode(plane, near, 1, k_step=k_step)[0]
        ix_of[near] = (s, gpu_ctx.build_index(s, 16))
    before, before_default = gpu_ctx.serial_launches(), pkg.default_serial_launches()
    for near, (s, ix) in ix_of.items():
        for bad in (2, 17, 0, 255):
            case = (near, bad)
            t = s[:14] + bytes([bad]) + s[15:]
            assert oracle.decode(t) is None, case
            assert gpu_ctx.decode_batch([t, t]) == [None, None], case
            assert pkg.decompress(t) is None, case
            d = gpu_ctx.decoder(4)
            d.feed(t, final=True)
            with pytest.raises(RuntimeError):
                d.info()
            with pytest.raises(RuntimeError):
                d.run()
            assert d.progress()["state"] == -1, case
            d.close()
            assert not pkg.check_index(ix, t) and not pkg.check_index(ix, t, gpu_ctx), case
            with pytest.raises(RuntimeError):
                gpu_ctx.build_index(t, 16)
            with pytest.raises(RuntimeError):
                gpu_ctx.decode_indexed(t, ix)
            # an index that names the step itself, every seal in order: head, entries, trailer
            count = struct.unpack_from("<i", ix, 40)[0]
            head = bytearray(ix[:96])
            struct.pack_into("<i", head, 28, bad)
            at, ents = 96, []
            for _ in range(count):
                n = struct.unpack_from("<Q", ix, at)[0]
                e = bytearray(ix[at + 8:at + 8 + n])
                struct.pack_into("<i", e, 28, bad)
                e[-32:] = hashlib.sha256(bytes(e[:-32])).digest()
                ents.append(bytes(e))
                at += 8 + n
            body = bytes(head) + b"".join(struct.pack("<Q", len(e)) + e for e in ents)
            forged = body + hashlib.sha256(body).digest()
            assert len(forged) == len(ix)
            assert not pkg.check_index(forged) and not pkg.check_index(forged, t), case
            assert not gpu_ctx.check_decoder_checkpoint(ents[0]), case
            with pytest.raises(RuntimeError):
                gpu_ctx.decoder(checkpoint=ents[0])
    assert gpu_ctx.serial_launches() == before, "a refused stream launched a kernel"
    assert pkg.default_serial_launches() == before_default, "a refused drop-in decode launched a kernel"
