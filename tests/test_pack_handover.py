"""GPU suite (-m gpu): the hand-over of coded bins in PACKS.  Up to eight images of a group launch are a pack: k_mix
leaves their 13-bit groups, k_pack_rows lays them side by side in a pack buffer, a coder thread takes one to three whole
packs and copies them chunk by chunk.  Every stream is compared byte for byte with the oracle's -n0 -e1 stream; the
contexts are small (n_slots <= 8, n_coders <= 2) and the images run from 1 x 1 to 300 x 400."""
import os
import subprocess
import sys

import numpy as np
import pytest

import inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ELEVEN = [("syn1", 300, 400), ("noise", 64, 64), ("const", 1, 1), ("ramp", 3, 5), ("syn1", 100, 77), ("noise", 37, 211),
          ("const", 120, 90), ("ramp", 256, 256), ("syn1", 17, 13), ("noise", 200, 150), ("ramp", 65, 63)]


def _images(cases):
    return [inputs.make(c, h, w) for c, h, w in cases]


@pytest.fixture(scope="module")
def eleven(oracle):
    imgs = _images(ELEVEN)
    return imgs, [oracle.encode(i, 0, 1)[0] for i in imgs]


@pytest.fixture(scope="module")
def simd(pkg):
    """The host's coder threads code packs only with AVX-512: without it every image goes on its own and none of these
    tests would reach the code they are about."""
    if pkg.range_code_multi([np.array([1], np.uint16)])[1] != 1:
        pytest.skip("no AVX-512 on this host: nothing is packed")
    return True


def test_mixed_pack_sizes(pkg, eleven, simd):
    """One group of eight slots: a pack of eight, then -- the first still queued, waiting for a second one -- a pack of three;
    one thread takes both."""
    imgs, want = eleven
    ctx = pkg.Context(device=0, n_slots=8, n_coders=2, n_groups=1)
    try:
        assert ctx.encode_batch(imgs) == want
        assert ctx.takes() == {11: 1}
    finally:
        ctx.close()


def test_two_images_then_one(pkg, eleven, simd):
    """A pack of two, then an image on its own (u16 records, the scalar coder).  (The take counts start again with every batch.)"""
    imgs, want = eleven
    ctx = pkg.Context(device=0, n_slots=2, n_coders=1, n_groups=1)
    try:
        assert ctx.encode_batch(imgs[:3]) == want[:3]
        assert ctx.takes() == {2: 1, 1: 1}
        assert ctx.encode_batch(imgs[3:4]) == want[3:4]          # a batch of one
        assert ctx.takes() == {1: 1}
        assert ctx.encode_batch(imgs[4:6]) == want[4:6]          # two images and one thread: two or fewer per thread, nothing is packed
        assert ctx.takes() == {1: 2}
    finally:
        ctx.close()


def test_three_pack_take(pkg, oracle, eleven, simd):
    """Twenty-five images through one group of four slots: packs of four, and the one coder thread waits for three of
    them each time; the twenty-fifth goes on its own."""
    imgs, want = eleven
    more = _images([("syn1", 40 + 3 * k, 50 + 7 * k) for k in range(14)])
    imgs, want = imgs + more, want + [oracle.encode(i, 0, 1)[0] for i in more]
    ctx = pkg.Context(device=0, n_slots=4, n_coders=1, n_groups=1)
    try:
        assert ctx.encode_batch(imgs) == want
        assert ctx.takes() == {12: 2, 1: 1}
    finally:
        ctx.close()
    ctx = pkg.Context(device=0, n_slots=4, n_coders=2, n_groups=1)       # two threads: which of them takes how many packs is a race, the bytes are not
    try:
        assert ctx.encode_batch(imgs) == want
        t = ctx.takes()
        assert set(t) <= {1, 4, 8, 12} and sum(k * v for k, v in t.items()) == 25 and t[1] == 1
    finally:
        ctx.close()


_CHILD = (
    "import importlib, sys, numpy as np\n"
    "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import torch; torch.cuda.init()\n"
    "import inputs\n"
    "from oracle.oracle import Oracle\n"
    "pkg = importlib.import_module('nblic-image-compression_amd')\n"
    "cases = %r\n"
    "imgs = [inputs.make(c, h, w) for c, h, w in cases]\n"
    "o = Oracle()\n"
    "want = [o.encode(i, 0, 1)[0] for i in imgs]\n"
    "ctx = pkg.Context(0, n_slots=8, n_coders=2, n_groups=1)\n"
    "got = ctx.encode_batch(imgs)\n"
    "for c, g, w in zip(cases, got, want):\n"
    "    assert g == w, c\n"
    "print('takes', sorted(ctx.takes().items()))\n"
    "ctx.debug_pack_rows(imgs[:3])\n"
    "ctx.close()\n"
    "print('live', sorted(pkg.live_resources().items()))\n"
    "print('child ok')\n"
)


def _child(env_extra):
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"), ELEVEN)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env_extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
    return r.stdout


def test_small_chunks(simd):
    """4096-bin chunks: the 300 x 400 image has some 500 thousand bins, so its lane runs through a hundred and more chunks,
    the ring's three slots are reused over and over and the other lanes end in chunks of their own."""
    out = _child({"NBLIC_AMD_CHUNK_BINS": "4096"})
    assert "takes [(11, 1)]" in out, out


def test_wide_positions(simd):
    """NBLIC_AMD_DBG=256: k_mix's plain 32-bit position path, packed."""
    out = _child({"NBLIC_AMD_DBG": "256"})
    assert "takes [(11, 1)]" in out, out


def test_layout(pkg, eleven):
    """One pack's device rows against pack_groups_host of the same images' u16 records (and those against the oracle's
    probabilities and bins)."""
    imgs, _ = eleven
    ctx = pkg.Context(device=0, n_slots=8, n_coders=2, n_groups=1)
    try:
        for lanes in (imgs[:8], imgs[8:11], imgs[2:4]):
            rows, coded = ctx.debug_pack_rows(lanes)
            assert len(coded) == len(lanes) and max(len(c) for c in coded) > 0
            want = pkg.pack_groups_host(coded)
            assert rows.shape == want.shape
            assert np.array_equal(rows, want)
    finally:
        ctx.close()


def test_records_of_the_layout_test_are_the_oracles(pkg, oracle, eleven):
    imgs, _ = eleven
    ctx = pkg.Context(device=0, n_slots=8, n_coders=2, n_groups=1)
    try:
        _, coded = ctx.debug_pack_rows(imgs[8:11])
        for img, rec in zip(imgs[8:11], coded):
            st = oracle.stages(img)
            assert np.array_equal(rec, st["prob"].astype(np.uint16) | (st["ev_bin"].astype(np.uint16) << 15))
    finally:
        ctx.close()


def test_resources():
    """In a process that has had this one context only: after close(), every count of nblic_amd_debug_live is zero -- pack
    buffers, pack rings and the debug hook's own pack included."""
    out = _child({})
    assert "live [('device', 0), ('locked', 0), ('pinned', 0), ('streams_events', 0)]" in out, out
