"""GPU suite (-m gpu): the chunks of coded-bin packs on a DMA engine (csrc/copy_engine.h).  One coder
thread and the smallest chunk the library accepts (4096 bins), so every take runs the three-slot ring round many times:
a 96 x 80 SYN-1 frame has some 34 thousand bins -- nine chunks -- and a 256 x 192 one over fifty.  Sizes and contents are
mixed inside a pack, so its lanes end in different chunks (the constant frames in the first).  Every stream is compared
byte for byte with the oracle's -n0 -e1 stream, with the engine on and off, and the counters say who carried the chunks.
An engine that is not available on the GPU machine is a FAILURE of these tests, not a skip."""
import os
import threading

import numpy as np
import pytest

import inputs

pytestmark = pytest.mark.gpu

SIZES = [(96, 80), (256, 192), (128, 100), (200, 150), (97, 81), (160, 191), (255, 96), (120, 192), (96, 192), (256, 80), (131, 177), (224, 99), (180, 180)]


def _cases(shift):
    """26 frames: the sizes above twice over, rotated by `shift`; every fifth frame constant, the rest SYN-1."""
    out = []
    for k in range(26):
        h, w = SIZES[(k + shift) % len(SIZES)]
        out.append(("const" if k % 5 == 2 else "syn1", h, w))
    return out


# name -> (frames, slots of the one group): twelve slots launch 12 + 12 + 2 frames, so the packs are 8, 4, 8, 4 and a LAST
# PACK OF TWO LANES (the pack of four still queued behind the thread's first take keeps the tail packed); eight slots
# launch 8 + 8 + 8 + 2, three full packs and two frames that go on their own through code_single, which stays with the runtime
BATCHES = {"last_pack_of_two": (_cases(0), 12), "full_packs_then_singles": (_cases(5), 8)}


@pytest.fixture(scope="module")
def simd(pkg):
    if pkg.range_code_multi([np.array([1], np.uint16)])[1] != 1:
        pytest.skip("no AVX-512 on this host: nothing is packed, so no chunk of a pack is ever copied")
    return True


@pytest.fixture(scope="module")
def batches(oracle):
    made = {}
    def plane(c, h, w):
        if (c, h, w) not in made:
            img = inputs.make(c, h, w)
            made[(c, h, w)] = (img, oracle.encode(img, 0, 1)[0])
        return made[(c, h, w)]
    return {name: ([plane(*c)[0] for c in cases], [plane(*c)[1] for c in cases], slots) for name, (cases, slots) in BATCHES.items()}


class _Env:
    """NBLIC_AMD_CHUNK_BINS and NBLIC_AMD_COPY_ENGINE are read when a context is created."""
    def __init__(self, engine):
        self.new = {"NBLIC_AMD_CHUNK_BINS": "4096", "NBLIC_AMD_COPY_ENGINE": "1" if engine else "0"}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.new}
        os.environ.update(self.new)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _encode(pkg, imgs, slots, engine):
    with _Env(engine):
        ctx = pkg.Context(device=0, n_slots=slots, n_coders=1, n_groups=1)
    try:
        got = ctx.encode_batch(imgs)
        return got, ctx.copy_stats(), ctx.takes()
    finally:
        ctx.close()


def test_the_engine_is_available_here(pkg, gpu_ctx):
    """Torch's HIP runtime brings libhsa-runtime64 into the process, and the library finds the eight entry points in it."""
    with _Env(True):
        ctx = pkg.Context(device=0, n_slots=2, n_coders=1)
    try:
        assert ctx.copy_stats() == {"engine": 0, "runtime": 0, "fallbacks": 0, "available": True}
    finally:
        ctx.close()


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_streams_with_the_engine_on_and_off(pkg, gpu_ctx, batches, simd, name):
    imgs, want, slots = batches[name]
    on, st_on, takes_on = _encode(pkg, imgs, slots, True)
    off, st_off, takes_off = _encode(pkg, imgs, slots, False)
    print(name, "engine on:", st_on, takes_on, "off:", st_off, takes_off)
    for k, (a, b, w) in enumerate(zip(on, off, want)):
        assert a == w, (name, k, "engine on")
        assert b == w, (name, k, "engine off")
    assert on == off
    assert st_on["available"] and st_on["engine"] > 0 and st_on["fallbacks"] == 0 and st_on["runtime"] == 0
    assert st_off["engine"] == 0 and st_off["fallbacks"] == 0 and not st_off["available"] and st_off["runtime"] == 0   # (off: not even opened, nothing counted)
    for takes in (takes_on, takes_off):
        assert sum(k * v for k, v in takes.items()) == 26
        if name == "last_pack_of_two":
            assert 1 not in takes, takes                              # nothing went on its own: the last two frames were a pack
    # every pack's longest lane spans at least seven chunks, and a take's chunks are those of its longest lane
    assert st_on["engine"] >= 7 * len(takes_on)


def test_two_contexts_at_once(pkg, gpu_ctx, batches, simd):
    """Two contexts, each with its own engine, signals and rings, encoding at the same time; after both close the library
    holds what it held before."""
    imgs, want, slots = batches["last_pack_of_two"]
    before = pkg.live_resources()
    with _Env(True):
        ctxs = [pkg.Context(device=0, n_slots=slots, n_coders=1, n_groups=1) for _ in range(2)]
    got, stats = [None, None], [None, None]
    try:
        assert pkg.live_resources()["streams_events"] >= before["streams_events"] + 2 * 3     # a signal per ring slot per coder thread at the least
        def run(i):
            got[i] = ctxs[i].encode_batch(imgs if i == 0 else imgs[::-1])
            stats[i] = ctxs[i].copy_stats()
        threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        for c in ctxs:
            c.close()
    assert got[0] == want and got[1] == want[::-1]
    for st in stats:
        assert st["available"] and st["engine"] > 0 and st["fallbacks"] == 0
    assert pkg.live_resources() == before
