"""GPU suite (-m gpu): the HIP path, called through the C ABI, against the oracle and the
committed golden fixtures.  Bit-exact is the bar for every stage and every stream."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def unpack_rec1(r):
    r = r.astype(np.uint32)
    px0 = r & 0xFF
    adr = (r >> 8) & 0x7FF
    qw = (r >> 19) & 31
    qu = (((r >> 16) & 7) << 1) | ((r >> 24) & 1)
    rel = (r >> 25) & 3
    qv = np.where(rel == 0, qu, np.where(rel == 1, qu + 1, qu - 1))
    return px0, adr, qu, qv, qw


def test_wave_primitives_selftest(gpu_ctx):
    assert gpu_ctx.selftest() == 0


STAGE_SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (17, 13), (40, 37), (64, 64), (96, 128), (5, 300)]


def _assert_stage_parity(gpu_ctx, oracle, img, content):
    """Every intermediate array of the staged -e1 pipeline for one image, against oracle.stages."""
    st = oracle.stages(img)
    px0, adr, qu, qv, qw = unpack_rec1(gpu_ctx.debug_stage(img, "rec1"))
    assert np.array_equal(px0, st["px0"]), ("px0", content)
    assert np.array_equal(adr, st["adr"]), ("adr", content)
    assert np.array_equal(qu, st["qu"]) and np.array_equal(qv, st["qv"]) and np.array_equal(qw, st["qw"]), ("level", content)
    pxs = gpu_ctx.debug_stage(img, "pxs")
    assert np.array_equal(pxs & 0xFF, st["px"]) and np.array_equal(pxs >> 8, st["sign"]), ("S2", content)
    assert np.array_equal(gpu_ctx.debug_stage(img, "z"), st["z"]), ("S3", content)
    assert np.array_equal(gpu_ctx.debug_stage(img, "cnt"), st["ev_count"]), ("S4 count", content)
    ev = gpu_ctx.debug_stage(img, "events")
    assert len(ev) == len(st["cu"])
    e_qu, e_qv, node = ev & 15, (ev >> 4) & 15, (ev >> 8) & 255
    assert np.array_equal(e_qu * 256 + node, st["cu"]) and np.array_equal(e_qv * 256 + node, st["cv"]), ("S4 path", content)
    assert np.array_equal((ev >> 16) & 31, st["ev_qw"]) and np.array_equal((ev >> 21) & 1, st["ev_bin"]), ("S4 bins", content)
    coded = gpu_ctx.debug_stage(img, "coded")
    assert np.array_equal(coded & 0xFFF, st["prob"]), ("S5 prob", content)
    assert np.array_equal(coded >> 15, st["ev_bin"]), ("S5 bin", content)
    return st


@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_stage_parity(gpu_ctx, oracle, shape):
    h, w = shape
    for content in ("syn1", "noise", "checker", "const", "ramp"):
        _assert_stage_parity(gpu_ctx, oracle, inputs.make(content, h, w), content)


def kodak_crops():
    """The 24 stored 64x96 Kodak crops (tests/golden/reference_fixtures.npz) and the reference's figures for them."""
    meta, arrays = inputs.fixtures()
    names = sorted(meta["kodak_crops"])
    return names, [np.ascontiguousarray(c) for c in arrays["kodak_crops"]], [meta["kodak_crops"][n] for n in names]


@pytest.mark.parametrize("content", ["kodak05_crop", "kodak_mosaic"])
def test_stage_parity_photographic(gpu_ctx, oracle, content):
    """Photographic pixels through every stage: one 64x96 crop, and a mosaic of 4 x 4 crops (256 x 384, 98304 pixels)
    whose counter chains run through many windows of 512 touches (the longest has 14836; asserted on the oracle's arrays,
    so that the mosaic cannot quietly stop being long enough).  A photograph spreads its pixels over the contexts: the
    longest context chain of the mosaic has 1452 records and stays inside one 4096-record block of k_bias_blocks; chains
    of several blocks are test_flat_and_structured_images_multi_block's."""
    _, crops, _ = kodak_crops()
    if content == "kodak05_crop":
        img = crops[4]
    else:
        img = np.ascontiguousarray(np.block([[crops[4 * r + c] for c in range(4)] for r in range(4)]))
        assert img.shape == (256, 384)
    st = _assert_stage_parity(gpu_ctx, oracle, img, content)
    if content == "kodak_mosaic":
        print("longest context chain", int(np.bincount(st["adr"], minlength=2048).max()), "records; longest counter chain",
              int(np.bincount(st["cu"], minlength=4096).max()), "touches")
        assert int(np.bincount(st["cu"], minlength=4096).max()) > 8 * 512


def test_kodak_crops_give_the_reference_hashes(gpu_ctx):
    """encode_batch / qencode_batch of the 24 stored crops: length and SHA-256 of the compiled reference's -e1 and -e0
    streams (tests/golden/reference_fixtures.json, make_fixtures.py) -- expected values that no code of ours produced."""
    names, crops, want = kodak_crops()
    assert len(crops) == 24 and crops[0].shape == (64, 96)
    got = gpu_ctx.encode_batch(crops)
    gotq = gpu_ctx.qencode_batch(crops)
    for name, s, q, m in zip(names, got, gotq, want):
        assert (len(s), sha(s)) == (m["len"], m["sha256"]), name
        assert (len(q), sha(q)) == (m["q_len"], m["q_sha256"]), name


def test_kodak_crops_every_mode(gpu_ctx, pkg, oracle):
    """The crops with inputs.PARAM_CLASSES cycled through encode_modes: streams and reconstructions against the oracle;
    then decode_batch of all of them and the band decoder on three."""
    names, crops, _ = kodak_crops()
    classes = [inputs.PARAM_CLASSES[k % len(inputs.PARAM_CLASSES)] for k in range(len(crops))]
    want = [oracle.encode(c, n, e) for c, (n, e) in zip(crops, classes)]
    streams, recs = gpu_ctx.encode_modes(crops, [c[0] for c in classes], [c[1] for c in classes])
    for name, s, r, w_, cl in zip(names, streams, recs, want, classes):
        assert s == w_[0], (name, cl)
        assert np.array_equal(r, w_[1]), (name, cl)
        assert int(np.abs(r.astype(int) - crops[names.index(name)].astype(int)).max()) <= w_[2], (name, cl)
    for name, g, w_, cl in zip(names, gpu_ctx.decode_batch(streams), want, classes):
        assert g is not None and np.array_equal(g[0], w_[1]) and g[1:] == (w_[2], w_[3]), (name, cl)
    for k, br in ((2, 1), (7, 5), (23, 0)):                               # (0, 3), (3, 3), (2, 2)
        assert np.array_equal(pkg.decompress_bands(streams[k], band_rows=br, chunk=1000, ctx=gpu_ctx), want[k][1]), (names[k], classes[k])


def test_batch_streams_equal_golden(gpu_ctx, golden):
    _, streams = golden
    imgs, want = [], []
    for (h, w) in inputs.SMALL_SHAPES:
        for content in inputs.CONTENTS:
            imgs.append(inputs.make(content, h, w))
            want.append(streams[inputs.case_id(content, h, w, 0, 1)].tobytes())
    got = gpu_ctx.encode_batch(imgs)
    for k, (g, wnt) in enumerate(zip(got, want)):
        assert g == wnt, k


def test_mixed_size_batch_equals_oracle(gpu_ctx, oracle):
    from oracle.oracle import syn1
    imgs = [syn1(512, 512, 1), inputs.make("noise", 300, 200), syn1(768, 512, 5), inputs.make("const", 1, 1),
            syn1(100, 1000, 3), inputs.make("checker", 257, 255), syn1(512, 768, 2)]
    got = gpu_ctx.encode_batch(imgs)
    for img, g in zip(imgs, got):
        assert g == oracle.encode(img, 0, 1)[0], img.shape


def test_flat_and_structured_images_multi_block(gpu_ctx, oracle):
    """Long context chains whose coupled warm-up cannot meet (constant error) must fall back to
    the in-order replay and still be exact; mixtures exercise both paths inside one chain."""
    half = inputs.make("const", 200, 300).copy()
    half[:, 150:] = inputs.make("noise", 200, 150)
    bands = inputs.make("ramp", 256, 256).copy()
    bands[64:192] = 200
    imgs = [inputs.make("const", 200, 300), inputs.make("ramp", 256, 256), inputs.make("checker", 300, 300), half, bands,
            np.zeros((130, 1000), np.uint8), np.full((500, 90), 255, np.uint8)]
    got = gpu_ctx.encode_batch(imgs)
    for k, (img, g) in enumerate(zip(imgs, got)):
        assert g == oracle.encode(img, 0, 1)[0], k


def test_touch_positions_packed_and_the_plain_32_bit_fallback(gpu_ctx, pkg, oracle):
    """k_touch_scatter hands k_mix 28-bit positions with qw / bin / parity in the spare bits; an image with 2^28 - 1
    touches or more (hundreds of megabins) keeps plain 32-bit positions and k_mix re-reads the events.  The fallback
    is forced here through the library's debug switch, in a process of its own (the switch is read once)."""
    WIDE_FLAG = 4                                             # kernels_e1.h kWideTouchFlag
    busy = pkg.syn1(1024, 1024, 3)
    assert gpu_ctx.debug_stage(busy, "totals")[WIDE_FLAG] == 0
    code = (
        "import importlib, sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch; torch.cuda.init()\n"
        "import inputs\n"
        "from oracle.oracle import Oracle\n"
        "pkg = importlib.import_module('nblic-image-compression_amd')\n"
        "ctx = pkg.Context(0, n_slots=4, n_coders=2)\n"
        "imgs = [pkg.syn1(700, 900, 5), inputs.make('noise', 300, 400), inputs.make('const', 200, 300), inputs.make('ramp', 256, 256)]\n"
        "assert ctx.debug_stage(imgs[0], 'totals')[4] == 1\n"
        "o = Oracle()\n"
        "for img, got in zip(imgs, ctx.encode_batch(imgs)):\n"
        "    assert got == o.encode(img, 0, 1)[0], img.shape\n"
        "print('wide ok')\n"
    ) % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, NBLIC_AMD_DBG="256")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "wide ok" in r.stdout, r.stdout + r.stderr


def test_output_capacity_is_enforced(gpu_ctx):
    img = inputs.make("noise", 64, 64)
    outs = [np.empty(600, np.uint8)]                      # noise needs > 4 KB
    with pytest.raises(RuntimeError):
        gpu_ctx.encode_ptrs([img.ctypes.data], [img.shape], False, outs)


def test_config2_4096_golden_and_round_trip(gpu_ctx, golden, oracle):
    """BASELINE config 2: 4096x4096 SYN-1, -n0 -e1.  Golden hash from the compiled reference;
    the stream must also decode (oracle decoder) back to the input."""
    from oracle.oracle import syn1
    manifest, _ = golden
    m = manifest["large"]["syn1s1_4096x4096_n0_e1"]
    img = syn1(4096, 4096, 1)
    assert sha(img.tobytes()) == m["input_sha256"]
    s = gpu_ctx.encode_batch([img])[0]
    assert len(s) == m["len"] == 8900446
    assert sha(s) == m["sha256"]
    dec = oracle.decode(s)
    assert dec is not None and np.array_equal(dec[0], img)


def test_gpu_decoders_at_baseline_sizes(gpu_ctx, pkg, golden):
    """The GPU decoders (k_serial_decode, k_serial_qdecode; resumable launches) on BASELINE-sized streams: the
    config-2 stream (4096 x 4096 -n0 -e1, 8,900,446 bytes, 77d18ede...) and the 4096 x 4096 effort-0 stream
    (ed712408...), both produced on the GPU and checked against the reference's golden hashes first, decoded in one
    nblic_amd_decode_batch call back to the input; then the config-2 stream through the drop-in NBLICdecompress,
    which fetches it on demand."""
    from oracle.oracle import syn1
    manifest, _ = golden
    img = syn1(4096, 4096, 1)
    s1 = gpu_ctx.encode_batch([img])[0]
    s0 = gpu_ctx.qencode_batch([img])[0]
    assert sha(s1) == manifest["large"]["syn1s1_4096x4096_n0_e1"]["sha256"] and sha(s0) == manifest["large"]["syn1s1_4096x4096_q0"]["sha256"]
    before = gpu_ctx.serial_launches()
    dec = gpu_ctx.decode_batch([s1, s0])
    assert gpu_ctx.serial_launches() - before >= 8                        # 4 Mpixel per launch: resumed launches, no kernel of tens of seconds
    assert dec[0] is not None and np.array_equal(dec[0][0], img) and dec[0][1:] == (0, 1)
    assert dec[1] is not None and np.array_equal(dec[1][0], img)
    d = pkg.decompress(s1)
    assert d is not None and np.array_equal(d[0], img)
    assert pkg.last_fed_bytes() <= len(s1) + (1 << 20) + 4 * 4096 + 1024


def test_config4_8192_n2e2_full_size(gpu_ctx, pkg, golden):
    """BASELINE config 4 at full size: 8192 x 8192 SYN-1, -n2 -e2 (near-lossless, least-squares predictor), worked
    through in row bands (nblic_amd_stream: bounded workspace, one model launch per band).  Stream 16,832,870 bytes,
    597d85ec... and the reconstruction (max error 2) from the compiled reference.  ~3 minutes."""
    from oracle.oracle import syn1
    manifest, _ = golden
    m = manifest["serial"]["syn1s1_8192x8192_n2_e2"]
    assert m["sha256"].startswith("597d85ec934d8b78") and m["len"] == 16832870
    img = syn1(8192, 8192, 1)
    ctx = pkg.Context(device=0, n_slots=2, n_coders=1)
    try:
        st = ctx.stream(img, 2, 2)
        done, s = st.run()
        prog = st.progress()
        rec, r0, r1 = st.recon()
        st.close()
    finally:
        ctx.close()
    assert done and (len(s), sha(s)) == (m["len"], m["sha256"]) and prog["sha256"] == m["sha256"]
    assert (r0, r1) == (0, 8192) and sha(rec.tobytes()) == m["recon_sha256"]
    assert int(np.abs(rec.astype(np.int16) - img.astype(np.int16)).max()) == 2


def test_device_resident_inputs(gpu_ctx, oracle):
    torch = pytest.importorskip("torch")
    from oracle.oracle import syn1
    imgs = [syn1(256, 384, s) for s in (1, 2, 3, 4)]
    dev = [torch.from_numpy(i).cuda() for i in imgs]
    torch.cuda.synchronize()
    outs, lens = gpu_ctx.encode_ptrs([d.data_ptr() for d in dev], [i.shape for i in imgs], True)
    for img, o, n in zip(imgs, outs, lens):
        assert o[:int(n)].tobytes() == oracle.encode(img, 0, 1)[0]


# ---- drop-in entry points, every mode (serial engine for everything but -n0 -e1) ------------
@pytest.mark.parametrize("near,effort", inputs.PARAM_CLASSES)
def test_dropin_compress_all_modes_small(pkg, golden, near, effort):
    manifest, streams = golden
    for (h, w) in [(1, 1), (1, 7), (7, 1), (3, 5), (17, 13)]:
        for content in ("syn1", "noise", "checker"):
            img = inputs.make(content, h, w)
            cid = inputs.case_id(content, h, w, near, effort)
            s, rec, n_out, e_out = pkg.compress(img, near, effort)
            assert s == streams[cid].tobytes(), cid
            m = manifest["small"][cid]
            assert (n_out, e_out) == (m["near_out"], m["effort_out"])
            assert sha(rec.tobytes()) == m["recon_sha256"], cid


@pytest.mark.parametrize("near,effort", [(0, 1), (2, 1), (0, 2), (3, 3)])
def test_dropin_decompress_reference_streams(pkg, golden, oracle, near, effort):
    _, streams = golden
    for (h, w) in [(1, 1), (2, 2), (5, 3), (17, 13), (64, 64) if effort == 1 else (17, 13)]:
        img = inputs.make("syn1", h, w)
        s = streams[inputs.case_id("syn1", h, w, near, effort)].tobytes()
        d = pkg.decompress(s)
        assert d is not None
        want = oracle.decode(s)
        assert np.array_equal(d[0], want[0]) and d[1:] == want[1:]
        assert int(np.abs(d[0].astype(int) - img.astype(int)).max()) <= near


def test_dropin_rejects_bad_input(pkg):
    assert pkg.decompress(b"Q0.2" + bytes(60)) is None                  # not an NBLIC stream
    assert pkg.compress(np.zeros((1, 1), np.uint8), 0, 1)[0] is not None


# ---- QNBLIC (effort 0): BASELINE config 1 on the GPU path -------------------------------------
def test_q_batch_streams_equal_golden(gpu_ctx, golden):
    _, streams = golden
    imgs, want = [], []
    for (h, w) in inputs.SMALL_SHAPES:
        for content in inputs.CONTENTS:
            imgs.append(inputs.make(content, h, w))
            want.append(streams[f"q_{content}_{h}x{w}"].tobytes())
    got = gpu_ctx.qencode_batch(imgs)
    for k, (g, wnt) in enumerate(zip(got, want)):
        assert g == wnt, k


def test_q_config1_512_and_4096_hashes(gpu_ctx, golden, oracle):
    """BASELINE config 1 (512x512 SYN-1, effort 0): golden 50fdb1a0...; and the 4096^2 frame."""
    from oracle.oracle import syn1
    manifest, _ = golden
    for key, hw in (("syn1s1_512x512_q0", 512), ("syn1s1_4096x4096_q0", 4096)):
        img = syn1(hw, hw, 1)
        s = gpu_ctx.qencode_batch([img])[0]
        assert len(s) == manifest["large"][key]["len"] and sha(s) == manifest["large"][key]["sha256"], key
    assert manifest["large"]["syn1s1_512x512_q0"]["sha256"].startswith("50fdb1a0a3cac171")
    small = syn1(300, 200, 3)
    s = gpu_ctx.qencode_batch([small, inputs.make("noise", 100, 333), inputs.make("const", 150, 150)])
    assert s[0] == oracle.qencode(small) and s[1] == oracle.qencode(inputs.make("noise", 100, 333))
    assert s[2] == oracle.qencode(inputs.make("const", 150, 150))


def test_q_dropin_round_trip(pkg, golden, oracle):
    _, streams = golden
    for (h, w) in [(1, 1), (1, 7), (7, 1), (3, 5), (17, 13), (64, 64), (2, 256)]:
        for content in ("syn1", "noise", "checker"):
            img = inputs.make(content, h, w)
            want = streams[f"q_{content}_{h}x{w}"].tobytes()
            assert pkg.qcompress(img) == want, (content, h, w)
            dec = pkg.qdecompress(want)                               # a stream the REFERENCE produced
            assert dec is not None and np.array_equal(dec, img), (content, h, w)
    assert pkg.qdecompress(b"NBLIC0.3" + bytes(40)) is None


def test_config3_kodak_shaped_batch(gpu_ctx, oracle):
    """BASELINE config 3: 24 images of Kodak's shapes (18 of 512x768 rows x cols... 768x512 and 6
    portrait), batched.  The Kodak files themselves never leave the build container, so the GPU
    box runs SYN-1 frames of the same shapes (seeds 1..24) against the oracle; parity of the
    oracle on the real Kodak pixels is pinned on the CPU side (test_oracle.py)."""
    from oracle.oracle import syn1
    shapes = [(512, 768)] * 18 + [(768, 512)] * 6
    imgs = [syn1(h, w, seed) for seed, (h, w) in enumerate(shapes, start=1)]
    got = gpu_ctx.encode_batch(imgs)
    gotq = gpu_ctx.qencode_batch(imgs[:6] + imgs[-3:])
    for k in range(24):                                                   # all 24, like the Kodak set itself on the CPU side
        assert got[k] == oracle.encode(imgs[k], 0, 1)[0], k
    assert len(set(got)) == 24
    for g, im in zip(gotq, imgs[:6] + imgs[-3:]):
        assert g == oracle.qencode(im)


@pytest.mark.parametrize("key", ["syn1s1_256x256_n0_e2", "syn1s1_256x256_n0_e3", "syn1s1_256x256_n2_e2", "syn1s1_512x512_n2_e1"])
def test_serial_modes_moderate_sizes(pkg, golden, oracle, key):
    """Stand-ins for BASELINE configs 4/5 (raster-serial modes) at sizes the serial engine finishes
    in seconds: stream and reconstruction hashes from the compiled reference, then a GPU decode."""
    from oracle.oracle import syn1
    manifest, _ = golden
    m = manifest["large"][key]
    name, dims, n, e = key.split("_")
    h, w = map(int, dims.split("x"))
    img = syn1(h, w, int(name[5:]))
    s, rec, _, _ = pkg.compress(img, int(n[1:]), int(e[1:]))
    assert (len(s), sha(s)) == (m["len"], m["sha256"])
    assert sha(rec.tobytes()) == m["recon_sha256"]
    d = pkg.decompress(s)
    assert d is not None and np.array_equal(d[0], rec) and d[1:] == (int(n[1:]), int(e[1:]))


def test_extreme_shapes_and_buffer_growth(gpu_ctx, oracle):
    """Maximum width / height (65535, NBLIC.h:29-30), and a noise frame whose 9.5 bins/px exceed the
    6 bins/px the event buffers are provisioned for (they are re-sized from the measured total)."""
    from oracle.oracle import syn1
    imgs = [syn1(1, 65535, 3), syn1(65535, 1, 4), syn1(3, 40000, 5), inputs.noise(1024, 1024, 11)]
    got = gpu_ctx.encode_batch(imgs)
    for k, (img, g) in enumerate(zip(imgs, got)):
        assert g == oracle.encode(img, 0, 1)[0], k
    gq = gpu_ctx.qencode_batch(imgs[:3])
    for img, g in zip(imgs[:3], gq):
        assert g == oracle.qencode(img)


def test_size_limits(pkg, gpu_ctx):
    # the reference refuses > 100,000,000 pixels (NBLIC.c:726): so do the drop-in symbols and the batch API
    big = np.zeros((1, 1), np.uint8)
    import ctypes as C
    lib = pkg.load_library()
    out = np.empty(64, np.uint8)
    n, e = C.c_int(0), C.c_int(1)
    u8p = C.POINTER(C.c_uint8)
    assert lib.NBLICcompress(0, out.ctypes.data_as(u8p), big.ctypes.data_as(u8p), 10001, 10000, C.byref(n), C.byref(e)) == -1
    assert lib.NBLICcompress(0, out.ctypes.data_as(u8p), big.ctypes.data_as(u8p), 0, 5, C.byref(n), C.byref(e)) == -1
    assert lib.QNBLICcompress(out.ctypes.data_as(C.POINTER(C.c_uint16)), big.ctypes.data_as(u8p), 70000, 1) == -1
    with pytest.raises(RuntimeError):
        gpu_ctx.encode_ptrs([big.ctypes.data], [(10001, 10000)], False, [np.empty(64, np.uint8)])


@pytest.mark.gpu
def test_sixteen_image_packs_and_chunked_streaming(pkg, oracle):
    """Many images, few coder threads: the coder threads take full 24-image sets (three AVX-512
    registers in lock-step; two for what is left at the end), stream each image's bins from HBM in chunks
    (256 Kbin here, so the images span up to a dozen chunks and all end at different bins) and wait for
    packs to fill mid-batch.  Every stream must still be the oracle's, byte for byte."""
    rng = np.random.default_rng(3)
    imgs = []
    for k in range(62):
        h, w = int(rng.integers(200, 760)), int(rng.integers(200, 900))
        imgs.append(inputs.make(inputs.CONTENTS[k % len(inputs.CONTENTS)], h, w) if k % 4 else inputs.syn1(h, w, seed=k + 1))
    import os
    os.environ["NBLIC_AMD_CHUNK_BINS"] = "262144"               # the pipeline's 4 Mbin chunks would swallow these images whole
    try:
        ctx = pkg.Context(device=0, n_slots=16, n_coders=2, n_groups=4, n_host_buffers=64)
    finally:
        del os.environ["NBLIC_AMD_CHUNK_BINS"]
    try:
        got = ctx.encode_batch(imgs)
        again = ctx.encode_batch(imgs[:5])                      # a short batch right after: singles
    finally:
        ctx.close()
    for k, (img, g) in enumerate(zip(imgs, got)):
        assert g == oracle.encode(img, 0, 1)[0], (k, img.shape)
    assert again == got[:5]


@pytest.mark.gpu
def test_production_shaped_context_many_small_images(pkg, oracle):
    """The bench's context shape (6 groups of 8, 16 coder threads, device-side backlog) fed 200
    images of every content and size class, twice over: all groups, driver threads, copy streams and
    coder threads are busy at once, packs form from images that end at wildly different bins."""
    rng = np.random.default_rng(17)
    imgs = []
    for k in range(200):
        h, w = int(rng.integers(1, 420)), int(rng.integers(1, 640))
        imgs.append(inputs.make(inputs.CONTENTS[k % len(inputs.CONTENTS)], h, w) if k % 3 else inputs.syn1(h, w, seed=k + 1))
    want = [oracle.encode(img, 0, 1)[0] for img in imgs]
    ctx = pkg.Context(device=0, n_slots=48, n_coders=16, n_groups=6, n_host_buffers=336)
    try:
        for _ in range(2):
            got = ctx.encode_batch(imgs)
            assert got == want
    finally:
        ctx.close()


@pytest.mark.gpu
def test_overlapping_batches_begin_end(pkg, oracle):
    """Three batches in flight at once (nblic_amd_encode_batch_begin / _end), ended out of order:
    every batch gets exactly its own streams."""
    rng = np.random.default_rng(23)
    batches = []
    for b in range(3):
        imgs = []
        for k in range(30):
            h, w = int(rng.integers(40, 500)), int(rng.integers(40, 600))
            imgs.append(inputs.make(inputs.CONTENTS[(k + b) % len(inputs.CONTENTS)], h, w) if k % 2 else inputs.syn1(h, w, seed=100 * b + k + 1))
        batches.append(imgs)
    ctx = pkg.Context(device=0, n_slots=12, n_coders=4, n_groups=3, n_host_buffers=64)
    try:
        tickets = [ctx.encode_begin([i.ctypes.data for i in imgs], [i.shape for i in imgs], False) for imgs in batches]
        results = {}
        for b in (1, 0, 2):
            outs, lens = ctx.encode_end(tickets[b])
            results[b] = [o[:int(n)].tobytes() for o, n in zip(outs, lens)]
        again = ctx.encode_batch(batches[0][:3])                 # the synchronous call still works afterwards
    finally:
        ctx.close()
    for b, imgs in enumerate(batches):
        assert results[b] == [oracle.encode(img, 0, 1)[0] for img in imgs], b
    assert again == results[0][:3]


# ---- serial modes: model stage one wave per image + parallel entropy stages; batch decoders ------
def test_serial_arithmetic_selftest(gpu_ctx):
    """The double-carried truncating divisions of the least-squares predictor (csrc/lsq_f64.h) against
    64-bit integer division, on the device."""
    assert gpu_ctx.serial_selftest() == 0


SERIAL_1024 = ["syn1s1_1024x1024_n0_e2", "syn1s1_1024x1024_n0_e3", "syn1s1_1024x1024_n2_e1", "syn1s1_1024x1024_n2_e2", "syn1s1_1024x1024_n9_e1"]
SERIAL_WIDE = ["syn1s1_64x16384_n0_e3", "syn1s1_24x16384_n2_e2", "syn1s1_16x16385_n0_e3", "syn1s1_3x20000_n0_e1", "syn1s1_3x20000_n2_e2",
               "syn1s1_3x20000_n1_e3", "syn1s1_8x16384_n3_e1", "syn1s1_6x16385_n2_e1", "syn1s1_512x512_n0_e2", "syn1s1_512x512_n0_e3",
               "syn1s1_512x512_n2_e2", "syn1s1_512x512_n1_e3"]


def _key_case(key):
    from oracle.oracle import syn1
    name, dims, n, e = key.split("_")
    h, w = map(int, dims.split("x"))
    return syn1(h, w, int(name[5:])), int(n[1:]), int(e[1:])


def test_serial_goldens_one_batch(pkg, golden):
    """SURVEY App. B's reference-held goldens at 1024^2 (n0e2 e9125b0c, n0e3 6c05e3cc, n2e1 05c22e7e, n2e2
    0323001d, n9e1 9c37cab5) plus wide strips around the 16384-pixel row (LDS row cache, 29 MB of
    statistics) and 512^2 frames: all in ONE batch, every image a wave of its own; then the streams are
    decoded in one batch and must give the reference's reconstruction."""
    manifest, _ = golden
    keys = SERIAL_1024 + SERIAL_WIDE
    cases = [_key_case(k) for k in keys]
    ctx = pkg.Context(device=0, n_slots=24, n_coders=4, n_groups=2, n_host_buffers=48)
    try:
        streams, recs = ctx.encode_modes([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
        dec = ctx.decode_batch(streams)
    finally:
        ctx.close()
    assert manifest["serial"]["syn1s1_1024x1024_n0_e2"]["sha256"].startswith("e9125b0c10fa1b51")
    assert manifest["serial"]["syn1s1_1024x1024_n0_e3"]["sha256"].startswith("6c05e3cc0745eb12")
    for key, s, rec, d, case in zip(keys, streams, recs, dec, cases):
        m = manifest["serial"][key]
        assert (len(s), sha(s)) == (m["len"], m["sha256"]), key
        assert sha(rec.tobytes()) == m["recon_sha256"], key
        assert d is not None and np.array_equal(d[0], rec) and (d[1], d[2]) == (case[1], case[2]), key


def test_serial_batch_many_images_in_flight(pkg, oracle):
    """160 images of every mode in one call (>= 128 in flight: 2 groups x 80 slots), mixed with -n0 -e1
    images that take the staged pipeline; every stream and reconstruction against the oracle; then one
    batch decode (NBLIC and QNBLIC streams mixed) against the oracle's decoders."""
    rng = np.random.default_rng(5)
    modes = [(0, 1), (0, 2), (0, 3), (1, 1), (2, 1), (2, 2), (9, 1), (3, 3), (5, 2), (1, 3)]
    imgs, nears, efforts = [], [], []
    for k in range(160):
        h, w = int(rng.integers(1, 70)), int(rng.integers(1, 90))
        imgs.append(inputs.make(inputs.CONTENTS[k % len(inputs.CONTENTS)], h, w) if k % 3 else inputs.syn1(h, w, seed=k + 1))
        nears.append(modes[k % len(modes)][0]); efforts.append(modes[k % len(modes)][1])
    ctx = pkg.Context(device=0, n_slots=160, n_coders=4, n_groups=2, n_host_buffers=200)
    try:
        streams, recs = ctx.encode_modes(imgs, nears, efforts)
        q = ctx.qencode_batch(imgs[:8])
        dec = ctx.decode_batch(streams + q + [b"NBLIC0.3" + bytes(30), b"junk"])
    finally:
        ctx.close()
    for k, (img, s, rec) in enumerate(zip(imgs, streams, recs)):
        ws, wrec, *_ = oracle.encode(img, nears[k], efforts[k])
        assert s == ws and np.array_equal(rec, wrec), (k, img.shape, nears[k], efforts[k])
        assert dec[k] is not None and np.array_equal(dec[k][0], wrec) and dec[k][1:] == (nears[k], efforts[k]), k
    for k in range(8):
        assert dec[160 + k] is not None and np.array_equal(dec[160 + k][0], imgs[k]), k
    assert dec[-2] is None and dec[-1] is None


def test_dropin_limit_is_opt_in(pkg):
    """The drop-in symbols refuse > 100,000,000 pixels (NBLIC.h:31) until the limit is raised for the
    context behind them (nblic_amd_set_max_pixels(NULL, ...)); a 3 x 40,000,000-pixel-wide frame cannot exist
    (65535 columns at most), so the check runs on the limit logic alone."""
    import ctypes as C
    lib = pkg.load_library()
    u8p = C.POINTER(C.c_uint8)
    img = np.zeros((2, 3), np.uint8)
    out = np.empty(4096, np.uint8)
    n, e = C.c_int(0), C.c_int(2)
    assert lib.NBLICcompress(0, out.ctypes.data_as(u8p), img.ctypes.data_as(u8p), 10001, 10000, C.byref(n), C.byref(e)) == -1
    pkg.set_default_max_pixels(5)
    try:
        assert lib.NBLICcompress(0, out.ctypes.data_as(u8p), img.ctypes.data_as(u8p), 2, 3, C.byref(n), C.byref(e)) == -1
    finally:
        pkg.set_default_max_pixels(0)
    assert lib.NBLICcompress(0, out.ctypes.data_as(u8p), img.ctypes.data_as(u8p), 2, 3, C.byref(n), C.byref(e)) > 0


def test_soak_random_contexts_and_batches(pkg, oracle):
    """Bounded soak (~20 rounds): random context shapes, chunk lengths, image sizes, contents and MODES,
    synchronous and overlapping batches, effort-0 batches and batch decodes through the same context."""
    import os
    rng = np.random.default_rng(20261004)
    modes = [(0, 1), (0, 1), (0, 1), (2, 1), (0, 2), (1, 3), (9, 1), (4, 2)]
    for rnd in range(20):
        groups, gsize, coders = int(rng.integers(1, 7)), int(rng.integers(1, 9)), int(rng.integers(1, 17))
        os.environ["NBLIC_AMD_CHUNK_BINS"] = str(int(rng.choice([4096, 10000, 65536, 262144, 1 << 22])))
        try:
            ctx = pkg.Context(device=0, n_slots=groups * gsize, n_coders=coders, n_groups=groups, n_host_buffers=int(rng.integers(8, 200)))
        finally:
            del os.environ["NBLIC_AMD_CHUNK_BINS"]
        try:
            batches = []
            for b in range(int(rng.integers(1, 4))):
                imgs = []
                for k in range(int(rng.integers(1, 40))):
                    big = rng.random() < 0.08
                    h, w = (int(rng.integers(300, 700)), int(rng.integers(300, 900))) if big else (int(rng.integers(1, 120)), int(rng.integers(1, 160)))
                    c = inputs.CONTENTS[int(rng.integers(0, len(inputs.CONTENTS)))]
                    imgs.append(inputs.make(c, h, w) if c != "syn1" else inputs.syn1(h, w, seed=int(rng.integers(1, 1000))))
                batches.append(imgs)
            if rng.random() < 0.5:
                tickets = [ctx.encode_begin([i.ctypes.data for i in imgs], [i.shape for i in imgs], False) for imgs in batches]
                for b in rng.permutation(len(batches)):
                    outs, lens = ctx.encode_end(tickets[b])
                    assert [x[:int(n)].tobytes() for x, n in zip(outs, lens)] == [oracle.encode(i, 0, 1)[0] for i in batches[b]], (rnd, b)
            else:
                for b, imgs in enumerate(batches):
                    small = [i for i in imgs if i.size <= 20000][:12] or imgs[:1]
                    md = [modes[int(rng.integers(0, len(modes)))] for _ in small]
                    streams, recs = ctx.encode_modes(small, [m[0] for m in md], [m[1] for m in md])
                    dec = ctx.decode_batch(streams)
                    for img, m, s, r, d in zip(small, md, streams, recs, dec):
                        ws, wrec, *_ = oracle.encode(img, m[0], m[1])
                        assert s == ws and np.array_equal(r, wrec) and d is not None and np.array_equal(d[0], wrec), (rnd, b, img.shape, m)
            if rng.random() < 0.3:
                q = batches[0][:6]
                assert ctx.qencode_batch(q) == [oracle.qencode(i) for i in q], rnd
        finally:
            ctx.close()


def test_device_coder_supplements_host_threads(pkg, oracle):
    """The range-coder stage on the GPU (one lane per image, 64 images per wave) next to ONE host coder
    thread: with a deep queue of finished images the pack threads take the newest 64 at a time.  Every
    stream -- host-coded or device-coded, all sizes and contents, images that end at very different bins
    inside one wave -- must be the oracle's, byte for byte; and an output buffer that is too small fails its own image alone."""
    rng = np.random.default_rng(41)
    imgs = []
    for k in range(420):
        h, w = int(rng.integers(1, 150)), int(rng.integers(1, 200))
        imgs.append(inputs.make(inputs.CONTENTS[k % len(inputs.CONTENTS)], h, w) if k % 3 else inputs.syn1(h, w, seed=k + 1))
    imgs[7] = inputs.syn1(700, 900, seed=5)                        # one long stream among short ones
    want = [oracle.encode(i, 0, 1)[0] for i in imgs]
    ctx = pkg.Context(device=0, n_slots=128, n_coders=1, n_groups=2, n_host_buffers=480)
    try:
        assert ctx.set_device_coder(2, 0) == 2
        got = ctx.encode_batch(imgs)
        stats = ctx.device_coder_stats()
        modes = ctx.encode_modes(imgs[:200], [2] * 200, [1] * 200)[0]      # serial-mode images go through the same queue
        # the same batch again, image 333's buffer one byte short (whether a host thread or the wave gets it is a race: the
        # kernel's own capacity checks are in test_device_coder.py): the call fails, that image has no length, every
        # other stream is whole, and the context goes on
        short = 333
        outs = [np.empty(pkg.out_capacity(*i.shape) if k != short else len(want[k]) - 1, np.uint8) for k, i in enumerate(imgs)]
        args = pkg._batch_args([i.ctypes.data for i in imgs], [i.shape for i in imgs], outs)
        rc = ctx.lib.nblic_amd_encode_batch(ctx.handle, len(imgs), args[0], 0, *args[1:])
        lens = list(args[5])
        after = ctx.encode_batch(imgs[300:364])
    finally:
        ctx.close()
    assert got == want
    assert modes == [oracle.encode(i, 2, 1)[0] for i in imgs[:200]]
    assert stats["images"] >= 64 and stats["packs"] >= 1, stats           # the device coder did take part
    assert rc != 0 and lens[short] < 0
    assert [o[:n].tobytes() for k, (o, n) in enumerate(zip(outs, lens)) if k != short] == want[:short] + want[short + 1:]
    assert after == want[300:364]


def test_serial_paths_at_extreme_widths_and_bad_streams(gpu_ctx, pkg, oracle):      # gpu_ctx first: torch must initialise HIP before the library does
    """Rows wider than the LDS row ring (taps then come from the reconstruction in memory): the encoder's
    model stage beyond ~50,000 columns, the decoders beyond ~24,000, up to the format's 65,535; device-resident
    inputs for the serial modes; and truncated / corrupt streams, which must come back as failures, never hang."""
    torch = pytest.importorskip("torch")
    cases = [(inputs.syn1(2, 65535, 3), 2, 1), (inputs.syn1(3, 52000, 4), 0, 2), (inputs.syn1(2, 30000, 5), 1, 3),
             (inputs.syn1(1, 65535, 6), 9, 1), (inputs.syn1(40, 700, 7), 3, 2)]
    ctx = pkg.Context(device=0, n_slots=8, n_coders=2, n_groups=2, n_host_buffers=16)
    try:
        streams, recs = ctx.encode_modes([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
        for (img, near, effort), s, rec in zip(cases, streams, recs):
            ws, wrec, *_ = oracle.encode(img, near, effort)
            assert s == ws and np.array_equal(rec, wrec), (img.shape, near, effort)
        q = ctx.qencode_batch([inputs.syn1(3, 40000, 8), inputs.syn1(2, 65535, 9)])
        dec = ctx.decode_batch(streams + q)
        for (img, near, effort), d, rec in zip(cases, dec, recs):
            assert d is not None and np.array_equal(d[0], rec) and d[1:] == (near, effort), img.shape
        assert np.array_equal(dec[-2][0], inputs.syn1(3, 40000, 8)) and np.array_equal(dec[-1][0], inputs.syn1(2, 65535, 9))
        # device-resident planes through the any-mode entry point
        import ctypes as C
        dev = [torch.from_numpy(c[0]).cuda() for c in cases[2:]]
        torch.cuda.synchronize()
        k = len(dev)
        outs = [np.empty(pkg.out_capacity(*c[0].shape), np.uint8) for c in cases[2:]]
        rr = [np.empty_like(c[0]) for c in cases[2:]]
        lens = (C.c_long * k)()
        rc = ctx.lib.nblic_amd_encode_batch_modes(
            ctx.handle, k, (C.c_void_p * k)(*[d.data_ptr() for d in dev]), 1,
            (C.c_int * k)(*[c[0].shape[0] for c in cases[2:]]), (C.c_int * k)(*[c[0].shape[1] for c in cases[2:]]),
            (C.c_int * k)(*[c[1] for c in cases[2:]]), (C.c_int * k)(*[c[2] for c in cases[2:]]),
            (C.c_void_p * k)(*[o.ctypes.data for o in outs]), (C.c_size_t * k)(*[o.size for o in outs]), lens,
            (C.c_void_p * k)(*[r.ctypes.data for r in rr]))
        assert rc == 0
        for j in range(k):
            assert outs[j][: lens[j]].tobytes() == streams[2 + j] and np.array_equal(rr[j], recs[2 + j])
        # damaged input
        good = streams[4]
        bad = [good[: len(good) * 6 // 10], good[:16], good[:20] + bytes(len(good) - 20), b"NBLIC0.3" + bytes(8),
               q[0][: len(q[0]) // 2], q[0][:8]]
        res = ctx.decode_batch(bad)
        assert res[0] is None and res[1] is None and res[3] is None and res[4] is None and res[5] is None
        assert res[2] is None or res[2][0].shape == (40, 700)          # zeros after the header may decode to SOMETHING, but must not hang
    finally:
        ctx.close()


def test_bench_two_ranks_on_one_gpu_rehearsal():
    """`bench.py --gpus 2` started directly: the launcher starts two ranks (both on GPU 0 here, gloo for the
    collectives), each encodes its own batch, the streams are gathered on rank 0; the line must say n_gpus 2,
    gathered_ok and bit_exact."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["NBLIC_BENCH_DEVICE"] = "0"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--height", "512", "--width", "512",
                        "--batch", "24", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["gathered_ok"] is True and line["bit_exact"] is True, line
    assert line["batch8_frames_per_gpu"] == 4
