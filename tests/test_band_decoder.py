"""GPU suite (-m gpu): the band decoder (nblic_amd_dstream_*, Context.decoder).  A stream of either codec is decoded
in row bands through a workspace sized by the band and the width, fed piece by piece, rows handed out as they finish,
suspended and resumed through checkpoints -- and every plane must equal the oracle's / the reference's, bit for bit."""
import hashlib
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

import inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def band_decode(ctx, stream, band_rows=0, rng=None, max_rows=0):
    """The whole stream through one decoder; pieces of random size when rng is given.  Returns (plane, progress)."""
    d = ctx.decoder(band_rows)
    parts, at = [], 0
    try:
        for _ in range(1_000_000):
            rc, rows, first = d.run(max_rows=max_rows)
            assert first == sum(p.shape[0] for p in parts)
            if rows.size:
                parts.append(rows)
            if rc == 1:
                break
            if rc == 2:
                n = int(rng.integers(1, 65537)) if rng is not None else len(stream)
                d.feed(stream[at:at + n], final=at + n >= len(stream))
                at += n
        prog = d.progress()
    finally:
        d.close()
    return np.concatenate(parts), prog


def expected(oracle, stream):
    return oracle.qdecode(stream) if stream[:1] == b"Q" else oracle.decode(stream)[0]


def _key_case(key):
    name, dims, n, e = key.split("_")
    h, w = map(int, dims.split("x"))
    return inputs.syn1(h, w, int(name[5:])), int(n[1:]), int(e[1:])


def test_goldens_every_codec_and_mode_random_pieces(gpu_ctx, golden, oracle):
    """All 450 small and 50 q_small golden streams, bands of 1 and 3 rows, fed in seeded random pieces."""
    manifest, streams = golden
    rng = np.random.default_rng(1234)
    keys = list(streams.keys())
    assert len(keys) == 500
    for key in keys:
        s = streams[key].tobytes()
        want = expected(oracle, s)
        assert want is not None, key
        for br in (1, 3):
            plane, prog = band_decode(gpu_ctx, s, br, rng)
            assert np.array_equal(plane, want), (key, br)
            assert prog["sha256"] == sha(plane.tobytes()) and prog["state"] == 1 and prog["rows_done"] == want.shape[0], (key, br)


CLASSES = [("n", 0, 1), ("n", 0, 2), ("n", 0, 3), ("n", 2, 1), ("n", 2, 2), ("n", 1, 3), ("n", 9, 1), ("q", 0, 0)]


def _class_stream(oracle, kind, near, effort, h=23, w=150, seed=5):
    img = inputs.syn1(h, w, seed)
    if kind == "q":
        s = oracle.qencode(img)
        return s, img
    s, rec, *_ = oracle.encode(img, near, effort)
    return s, rec


def test_checkpoint_after_every_band_resumes_on_a_second_context(gpu_ctx, pkg, oracle):
    ctx2 = pkg.Context(device=0, n_slots=1, n_coders=1)
    try:
        for kind, near, effort in CLASSES:
            s, rec = _class_stream(oracle, kind, near, effort)
            br = 4
            d = gpu_ctx.decoder(br)
            d.feed(s, final=True)
            done = []
            while True:
                rc, rows, first = d.run(max_rows=br)
                done.append(rows)
                if rc == 1:
                    break
                assert rc == 0
                ck = d.checkpoint()
                prog = d.progress()
                assert gpu_ctx.check_decoder_checkpoint(ck)
                r = ctx2.decoder(checkpoint=ck)
                r.feed(s[prog["feed_from"]:], final=True)
                rc2, rest, first2 = r.run()
                assert rc2 == 1 and first2 == prog["rows_done"]
                plane = np.concatenate(done + [rest])
                assert np.array_equal(plane, rec), (kind, near, effort, first2)
                assert r.progress()["sha256"] == sha(rec.tobytes())
                r.close()
            d.close()
            assert np.array_equal(np.concatenate(done), rec), (kind, near, effort)
    finally:
        ctx2.close()


_CHILD = r"""
import importlib, sys
sys.path.insert(0, sys.argv[1])
pkg = importlib.import_module("nblic-image-compression_amd")
ck = open(sys.argv[2], "rb").read(); s = open(sys.argv[3], "rb").read()
ctx = pkg.Context(device=0, n_slots=1, n_coders=1)
d = ctx.decoder(checkpoint=ck)
ff = d.progress()["feed_from"]
d.feed(s[ff:], final=True)
rc, rows, first = d.run()
assert rc == 1
print(first, d.progress()["sha256"])
ctx.close()
"""


def test_resume_in_a_fresh_process(gpu_ctx, oracle):
    s, rec = _class_stream(oracle, "n", 0, 3, h=30, w=200)
    d = gpu_ctx.decoder(7)
    d.feed(s, final=True)
    rc, rows, _ = d.run(max_rows=7)
    rc, rows2, _ = d.run(max_rows=7)
    assert rc == 0
    ck = d.checkpoint()
    d.close()
    with tempfile.TemporaryDirectory() as t:
        open(os.path.join(t, "ck"), "wb").write(ck)
        open(os.path.join(t, "s"), "wb").write(s)
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(t, "ck"), os.path.join(t, "s")],
                           capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    first, digest = r.stdout.split()[-2:]
    assert int(first) == 14 and digest == sha(rec.tobytes())


def test_damaged_checkpoints_and_streams_are_refused(gpu_ctx, pkg, oracle):
    s, rec = _class_stream(oracle, "n", 2, 2, h=20, w=120)
    d = gpu_ctx.decoder(5)
    d.feed(s, final=True)
    assert d.run(max_rows=5)[0] == 0
    ck = d.checkpoint()
    d.close()
    gpu_ctx.decoder(checkpoint=ck).close()                          # the undamaged one is taken

    def flip(b, at):
        b = bytearray(b)
        b[at] ^= 0x10
        return bytes(b)

    version_bumped = bytearray(ck)
    version_bumped[8] += 1
    version_bumped[-32:] = hashlib.sha256(bytes(version_bumped[:-32])).digest()     # a consistent checksum: the version alone refuses it
    bad = {"header": flip(ck, 16), "body": flip(ck, len(ck) // 2), "checksum": flip(ck, len(ck) - 1),
           "truncated": ck[:-1], "version": bytes(version_bumped), "empty": b"", "junk": bytes(len(ck))}
    for name, b in bad.items():
        assert not gpu_ctx.check_decoder_checkpoint(b), name
        with pytest.raises(RuntimeError):
            gpu_ctx.decoder(checkpoint=b)
    # a truncated stream marked final fails, it does not hang
    d = gpu_ctx.decoder(3)
    d.feed(s[: len(s) // 2], final=True)
    t0 = time.time()
    with pytest.raises(RuntimeError):
        while True:
            rc, _, _ = d.run()
            assert rc != 1
    assert time.time() - t0 < 30
    d.close()
    # an unfed decoder asks for input; fed, it goes on
    d = gpu_ctx.decoder(3)
    rc, rows, first = d.run()
    assert rc == 2 and rows.shape[0] == 0 and d.info() is None
    d.feed(s[:40])
    assert d.run()[0] == 2
    d.feed(s[40:], final=True)
    rc, rows, first = d.run()
    assert rc == 1 and first == 0 and np.array_equal(rows, rec)
    d.close()


def test_wide_rows_take_the_uncached_paths(gpu_ctx, oracle):
    img = inputs.syn1(12, 40000, 3)
    for near, effort in ((0, 3), (2, 1)):
        s, rec, *_ = oracle.encode(img, near, effort)
        plane, prog = band_decode(gpu_ctx, s, 3, np.random.default_rng(near))
        assert np.array_equal(plane, rec), (near, effort)
    q = oracle.qencode(img)
    plane, _ = band_decode(gpu_ctx, q, 5, np.random.default_rng(9))
    assert np.array_equal(plane, img)


STRIPS = ["syn1s1_64x16384_n0_e3", "syn1s1_24x16384_n2_e2", "syn1s1_8x16384_n3_e1", "syn1s1_6x16385_n2_e1", "syn1s1_3x20000_n1_e3"]


def _split_decode(pkg, ctx, s, band_rows):
    """First band on ctx, checkpoint, the rest on a second Context: returns the running row hash."""
    d = ctx.decoder(band_rows)
    d.feed(s, final=True)
    rc, rows, _ = d.run(max_rows=band_rows)
    if rc == 1:
        digest = d.progress()["sha256"]
        d.close()
        return digest
    assert rc == 0
    ck, ff = d.checkpoint(), d.progress()["feed_from"]
    d.close()
    ctx2 = pkg.Context(device=0, n_slots=1, n_coders=1)
    try:
        r = ctx2.decoder(checkpoint=ck)
        r.feed(s[ff:], final=True)
        while True:
            rc, _, _ = r.run()
            if rc == 1:
                break
            assert rc == 0
        return r.progress()["sha256"]
    finally:
        ctx2.close()


def test_golden_strips_across_a_checkpoint(gpu_ctx, pkg, golden):
    manifest, _ = golden
    cases = [_key_case(k) for k in STRIPS]
    streams, _ = gpu_ctx.encode_modes([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], want_recon=False)
    for key, s, (img, near, effort) in zip(STRIPS, streams, cases):
        m = manifest["serial"][key]
        assert (len(s), sha(s)) == (m["len"], m["sha256"]), key
        assert _split_decode(pkg, gpu_ctx, s, max(1, img.shape[0] // 3)) == m["recon_sha256"], key


def test_config5_slice_1024x16384_n0_e3(pkg, golden):
    """16.8 Mpixel at -n0 -e3: encoded (its hash against the manifest), then band-decoded in two run calls on two
    Contexts with a checkpoint between them; the row hash must be the reference's reconstruction hash."""
    manifest, _ = golden
    key = "syn1s1_1024x16384_n0_e3"
    m = manifest["serial"][key]
    img, near, effort = _key_case(key)
    ctx = pkg.Context(device=0, n_slots=2, n_coders=2)
    try:
        streams, _ = ctx.encode_modes([img], [near], [effort], want_recon=False)
        s = streams[0]
        assert (len(s), sha(s)) == (m["len"], m["sha256"])
        d = ctx.decoder(0)
        d.feed(s, final=True)
        rc, rows, _ = d.run(max_rows=512)
        assert rc == 0 and rows.shape[0] == 512
        ck, ff = d.checkpoint(), d.progress()["feed_from"]
        d.close()
    finally:
        ctx.close()
    ctx2 = pkg.Context(device=0, n_slots=1, n_coders=1)
    try:
        r = ctx2.decoder(checkpoint=ck)
        r.feed(s[ff:], final=True)
        rc, rows, first = r.run()
        assert rc == 1 and first == 512 and rows.shape[0] == 512
        assert r.progress()["sha256"] == m["recon_sha256"]
    finally:
        ctx2.close()


def test_device_memory_does_not_depend_on_the_height(gpu_ctx, oracle):
    out = {}
    for kind, near, effort in (("n", 0, 1), ("n", 0, 3), ("q", 0, 0)):
        for h in (64, 1024):
            img = inputs.syn1(h, 4096, 2)
            s = oracle.qencode(img) if kind == "q" else oracle.encode(img, near, effort)[0]
            d = gpu_ctx.decoder(16)
            d.feed(s[:70000])
            assert d.info() is not None
            out[(kind, effort, h)] = d.progress()["device_bytes"]
            d.close()
        assert out[(kind, effort, 64)] == out[(kind, effort, 1024)], out
        br, w = 16, 4096
        stride = {3: 128, 2: 64}.get(effort, 0)
        win = max(4 << 20, 2 * br * w + 8 * w + 2048) + 511 + 2048
        bound = (br + 2) * w + 2 * w + win + 90 * 1024 + 1024 + 3 * w * stride * 8 + 24576
        assert out[(kind, effort, 64)] <= bound, (kind, effort, out)


def test_no_slower_than_the_one_call_decoder(gpu_ctx, pkg, oracle):
    """The band decoder, and the drop-in decoder that runs it, against the whole-plane decoder: a one-image
    decode_batch launches the same non-lean kernel with the same rows per launch."""
    img = inputs.syn1(64, 16384, 1)
    s, rec, *_ = oracle.encode(img[:4], 0, 3)                       # warm every path up on a small stream
    gpu_ctx.decode_batch([s])
    pkg.decompress(s)
    band_decode(gpu_ctx, s)
    streams, _ = gpu_ctx.encode_modes([img], [0], [3], want_recon=False)
    s = streams[0]
    t0 = time.perf_counter()
    one = gpu_ctx.decode_batch([s])[0]
    t_one = time.perf_counter() - t0
    t0 = time.perf_counter()
    plane, _ = band_decode(gpu_ctx, s)
    t_band = time.perf_counter() - t0
    t0 = time.perf_counter()
    dropin = pkg.decompress(s)
    t_dropin = time.perf_counter() - t0
    assert np.array_equal(one[0], img) and np.array_equal(plane, img) and np.array_equal(dropin[0], img)
    print(f"decode_batch {t_one:.3f} s, band decoder {t_band:.3f} s, drop-in {t_dropin:.3f} s")
    assert t_band <= 1.15 * t_one and t_dropin <= 1.15 * t_one, (t_band, t_dropin, t_one)


def test_coexists_with_band_encoder_and_decode_batch(gpu_ctx, oracle):
    dimg = inputs.syn1(40, 900, 11)
    ds, drec, *_ = oracle.encode(dimg, 1, 2)
    eimg = inputs.syn1(48, 700, 12)
    es_want = oracle.encode(eimg, 0, 3)[0]
    mix = [oracle.encode(inputs.syn1(30, 200, 20 + k), k % 3, 1 + k % 3)[0] for k in range(6)] + \
          [oracle.qencode(inputs.syn1(25, 180, 30 + k)) for k in range(3)]
    mix_want = [expected(oracle, m) for m in mix]
    dec = gpu_ctx.decoder(4)
    dec.feed(ds, final=True)
    enc = gpu_ctx.stream(eimg, 0, 3, band_rows=6)
    parts, pieces = [], []
    dec_done = enc_done = False
    for _ in range(100):
        if not dec_done:
            rc, rows, _ = dec.run(max_rows=4)
            parts.append(rows)
            dec_done = rc == 1
        if not enc_done:
            enc_done, b = enc.run(budget_seconds=1e-6)
            pieces.append(b)
        got = gpu_ctx.decode_batch(mix)
        for g, want in zip(got, mix_want):
            assert g is not None and np.array_equal(g[0], want)
        if dec_done and enc_done:
            break
    dec.close()
    enc.close()
    assert np.array_equal(np.concatenate(parts), drec)
    assert b"".join(pieces) == es_want


def test_integer_redo_in_random_pieces_and_on_wide_rows(gpu_ctx, pkg, oracle):
    """Hard-edged planes coded near-lossless send pixels of efforts 2 / 3 to the integer redo of the least squares
    (test_gpu_resume.py test_integer_redo_runs_in_every_kernel_variant).  The band decoder, fed in seeded random pieces,
    bands of 5 rows: the oracle's plane, and the device counted redone pixels; the same for a row too wide for the LDS row
    cache (30000 pixels, an edge every 64: the decoder that reads its taps from memory), which syn1 never does."""
    # (nblic_amd_serial_plan: the launchers' own decision) 64 pixels are cached in LDS, 30000 are not; one stream is never lean
    assert pkg.serial_plan(True, 2, 1, 64, False) == pkg.PLAN_ROWS_IN_LDS and pkg.serial_plan(True, 3, 1, 64, False) == pkg.PLAN_ROWS_IN_LDS
    assert pkg.serial_plan(True, 2, 1, 30000, False) == 0 and pkg.serial_plan(True, 3, 1, 30000, False) == 0
    for name, h, w, br in (("step_v", 64, 64, 5), ("bars_v", 6, 30000, 3)):
        img = inputs.make_hard(name, h, w)
        for near, effort in ((2, 2), (2, 3)):
            s, rec, *_ = oracle.encode(img, near, effort)
            gpu_ctx.lsq_redo_counts(reset=True)
            plane, prog = band_decode(gpu_ctx, s, br, np.random.default_rng(near + effort))
            assert np.array_equal(plane, rec) and prog["sha256"] == sha(plane.tobytes()), (name, near, effort)
            c = gpu_ctx.lsq_redo_counts(reset=True)
            print(f"lsq redo on the device: band decoder{' uncached' if w > 20000 else ''} {name} {h}x{w} -n{near} -e{effort}: system 0 {c[0]}, system 1 {c[1]}")
            assert c[0] >= 1, (name, near, effort)
