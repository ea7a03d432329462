"""GPU suite: the device rANS stage of effort 0 (csrc/q_device_coder.hip, k_q_rans_lanes) on its own, lane by lane against
the host stage.  ``debug_device_q_entropy`` runs a resumed launch sequence on caller-made jobs whose output regions are
followed by guards; every lane must give the bytes of ``q_entropy_entries`` (held to the reference by the CPU suite)."""
import numpy as np
import pytest

import inputs

import qcoder_inputs as qi

pytestmark = pytest.mark.gpu

# 70002, not the 70001 one would pick: 70001 is prime, so no header of two 16-bit sides names an image of that many pixels and
# q_entropy_entries (the reference here) cannot code one.  70002 = 2 x 35001: as far from a multiple of 256, 274 windows.
LENGTHS = (1, 3, 255, 256, 257, 511, 513, 4097, 70002)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(device=0, n_slots=2, n_coders=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def jobs(pkg):
    """130 jobs, ragged: job k has LENGTHS[k % 9] symbols, so every wave mixes one-symbol jobs with 70002-symbol ones that
    finish many launches later; the constructions (uniform, f = 1 runs, f = 32767 runs) rotate.  (words, hist, padded, stream)."""
    out = []
    for k in range(130):
        n = LENGTHS[k % len(LENGTHS)]
        words, hist = qi.job(n, k)
        want = pkg.q_entropy_entries(words.reshape(pkg.q_hook_shape(n)), (), hist)[0]
        assert want is not None
        out.append((words, hist, qi.padded(words, 1000 + k), want))
    return out


def test_quotient_selftest(ctx):
    assert ctx.qcoder_selftest() == 0


@pytest.mark.parametrize("budget", (64, 257, 0))
@pytest.mark.parametrize("count", (1, 63, 64, 65, 130))
def test_lanes_match_the_host_stage(ctx, jobs, count, budget):
    first = 8 if count == 1 else 0                                   # a lone job: the longest
    sel = jobs[first:first + count]
    if budget == 64:                                                 # 1094 launches for 70002 symbols: keep the long jobs to one per wave
        sel = [j for i, j in enumerate(sel, first) if len(j[0]) < 70002 or i % 64 == 8]
    got = ctx.debug_device_q_entropy([(p, len(w), h, len(s) // 2) for w, h, p, s in sel], budget)      # capacities that fit exactly
    for k, (g, j) in enumerate(zip(got, sel)):
        assert g == j[3], (k, len(j[0]))


def test_capacity_one_word_short_costs_that_lane_alone(ctx, jobs):
    sel = jobs[:65]
    short = {2, 17, 35, 64}                                          # lengths 255, 70002, 70002, 3
    got = ctx.debug_device_q_entropy([(p, len(w), h, len(s) // 2 - (k in short)) for k, (w, h, p, s) in enumerate(sel)], 257)
    for k, (g, j) in enumerate(zip(got, sel)):
        assert g == (None if k in short else j[3]), k


def test_capacity_zero_and_front_matter_only(ctx, jobs):
    sel = jobs[:10]
    front = [len(s) // 2 - 2 for w, h, p, s in sel]                  # room for less than the flush: at most the front matter fits
    caps = [0, 1, 5] + front[3:]
    got = ctx.debug_device_q_entropy([(p, len(w), h, c) for (w, h, p, s), c in zip(sel, caps)], 0)
    assert got == [None] * 10


def test_hook_refuses_bad_words(ctx, jobs):
    w, h, p, s = jobs[4]
    bad = p.copy()
    bad[0] = 12
    with pytest.raises(ValueError):
        ctx.debug_device_q_entropy([(bad, len(w), h, len(s) // 2)], 0)
    with pytest.raises(ValueError):
        ctx.debug_device_q_entropy([(p[:200], len(w), h, len(s) // 2)], 0)


# ---- in the pipeline: on launch_q's coded-bin buffers, the pad word and the raw histogram behind the last pixel ----------
@pytest.fixture(scope="module")
def batch(oracle, golden):
    """The images of the QNBLIC parity test (every small shape, every content) plus 1x1, 1x300 and 257x255, with the
    reference's streams: the goldens where there is one, the oracle for the three extra sizes."""
    _, streams = golden
    imgs, want = [], []
    for (h, w) in inputs.SMALL_SHAPES:
        for content in inputs.CONTENTS:
            imgs.append(inputs.make(content, h, w))
            want.append(streams[f"q_{content}_{h}x{w}"].tobytes())
    for content, h, w in (("noise", 1, 1), ("syn1", 1, 300), ("noise", 257, 255), ("syn1", 257, 255)):
        imgs.append(inputs.make(content, h, w))
        want.append(oracle.qencode(imgs[-1]))
    return imgs, want


def test_pipeline_device_mode(pkg, batch, oracle):
    imgs, want = batch
    before = pkg.live_resources()
    c = pkg.Context(device=0, n_slots=4, n_coders=2)
    try:
        host = c.qencode_batch(imgs)                                 # mode 0, the default
        assert c.device_qcoder_stats()["images"] == 0
        assert c.set_device_qcoder(1, 300) == 1
        got = c.qencode_batch(imgs)
        stats = c.device_qcoder_stats()
        assert got == host and got == want
        assert stats["images"] == len(imgs) and stats["launches"] > 1
        assert stats["symbols"] == sum(i.size for i in imgs)
        # an output buffer one word too small: -1 for that image alone
        planes = [np.ascontiguousarray(i) for i in imgs[-6:]]
        outs = [np.empty(len(w) // 2 - (k == 2), np.uint16) for k, w in enumerate(want[-6:])]
        with pytest.raises(RuntimeError):
            c.qencode_ptrs([p.ctypes.data for p in planes], [p.shape for p in planes], False, outs)
        outs[2] = np.empty(len(want[-4]) // 2, np.uint16)
        o, lens = c.qencode_ptrs([p.ctypes.data for p in planes], [p.shape for p in planes], False, outs)
        assert [a[:int(n)].tobytes() for a, n in zip(o, lens)] == want[-6:]
        # shared mode: the same bytes, whoever codes which image
        assert c.set_device_qcoder(2, 300) == 2
        assert c.qencode_batch(imgs) == want
        # an -e1 batch on the same context afterwards
        assert c.set_device_qcoder(1, 300) == 1
        e1 = imgs[-8:]
        assert c.encode_batch(e1) == [oracle.encode(i, 0, 1)[0] for i in e1]
        assert c.set_device_qcoder(0) == 0
        assert c.qencode_batch(imgs[:5]) == want[:5]
        assert c.device_qcoder_stats()["images"] >= len(imgs) + 12              # the batch and the two calls of six; what shared mode took is a race
    finally:
        c.close()
    assert pkg.live_resources() == before


def test_one_word_short_reports_that_image_alone(pkg, batch):
    """The lengths array of the failed call: -1 for the short image, the true lengths for the others."""
    import ctypes as C
    imgs, want = batch
    c = pkg.Context(device=0, n_slots=4, n_coders=2)
    try:
        c.set_device_qcoder(1, 300)
        planes = [np.ascontiguousarray(i) for i in imgs[-5:]]
        k = len(planes)
        outs = [np.empty(len(w) // 2 - (j == 3), np.uint16) for j, w in enumerate(want[-5:])]
        lens = (C.c_long * k)()
        rc = c.lib.nblic_amd_qencode_batch(
            c.handle, k, (C.c_void_p * k)(*[p.ctypes.data for p in planes]), 0, (C.c_int * k)(*[p.shape[0] for p in planes]),
            (C.c_int * k)(*[p.shape[1] for p in planes]), (C.c_void_p * k)(*[o.ctypes.data for o in outs]), (C.c_size_t * k)(*[o.size for o in outs]), lens)
        assert rc != 0
        assert list(lens) == [len(w) // 2 if j != 3 else -1 for j, w in enumerate(want[-5:])]
        for j in (0, 1, 2, 4):
            assert outs[j].tobytes() == want[-5:][j]
    finally:
        c.close()


def test_dropin_device_mode(pkg, golden):
    _, streams = golden
    assert pkg.set_device_qcoder(None, 1) == 1
    try:
        for content, h, w in (("syn1", 64, 64), ("noise", 17, 13), ("checker", 1, 1), ("syn1", 2, 256)):
            assert pkg.qcompress(inputs.make(content, h, w)) == streams[f"q_{content}_{h}x{w}"].tobytes(), (content, h, w)
    finally:
        assert pkg.set_device_qcoder(None, 0) == 0
