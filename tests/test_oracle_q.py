"""CPU suite: pins the oracle's QNBLIC (effort 0) restatement to the reference -- committed q_*
golden streams, live comparison when oracle/_ref is present, and the closed-form neighbourhood
(what a stateless GPU kernel needs) against the reference's running window."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import inputs


def test_q_golden_streams(oracle, golden):
    manifest, streams = golden
    for (h, w) in inputs.SMALL_SHAPES:
        for content in inputs.CONTENTS:
            img = inputs.make(content, h, w)
            want = streams[f"q_{content}_{h}x{w}"].tobytes()
            assert oracle.qencode(img) == want, (content, h, w)
            dec = oracle.qdecode(want)
            assert dec is not None and np.array_equal(dec, img), (content, h, w)


def test_q_known_answer_1x1(oracle):
    # 1x1 image, pixel 77 -> 62 bytes
    s = oracle.qencode(np.array([[77]], np.uint8))
    assert len(s) == 62 and s[:14].hex() == "51302e320100010062e0ff7f00d2" and s[-4:].hex() == "01000200"


@pytest.mark.parametrize("key", ["syn1s1_512x512_q0"])
def test_q_large_hash(oracle, golden, key):
    from oracle.oracle import syn1
    manifest, _ = golden
    s = oracle.qencode(syn1(512, 512, 1))
    assert len(s) == manifest["large"][key]["len"] and hashlib.sha256(s).hexdigest() == manifest["large"][key]["sha256"]


def test_q_closed_form_neighbourhood_equals_window(oracle):
    lib = oracle.lib
    rng = np.random.default_rng(3)
    for h in range(1, 7):
        for w in range(1, 10):
            img = rng.integers(0, 256, (h, w), dtype=np.uint8)
            win = np.zeros(h * w * 11, np.int32)
            lib.orc_q_taps_window(img.ctypes.data_as(C.POINTER(C.c_uint8)), h, w, win.ctypes.data_as(C.POINTER(C.c_int)))
            win = win.reshape(h, w, 11)
            one = np.zeros(11, np.int32)
            for i in range(h):
                for j in range(w):
                    lib.orc_q_taps(img.ctypes.data_as(C.POINTER(C.c_uint8)), w, i, j, one.ctypes.data_as(C.POINTER(C.c_int)))
                    assert np.array_equal(one, win[i, j]), (h, w, i, j, one, win[i, j])


def test_q_vs_live_reference(oracle):
    """Random shapes: the reference's streams stored in tests/golden/reference_fixtures.* (make_fixtures.py), and the
    compiled reference itself wherever oracle/_ref was built."""
    from oracle.oracle import Reference
    _, stored = inputs.fixtures()
    reference = Reference() if Reference.available() else None
    cases = inputs.random_q_cases()
    for k, img in enumerate(cases):
        a = oracle.qencode(img)
        assert a == stored[f"q_case_{k}"].tobytes(), img.shape
        assert np.array_equal(oracle.qdecode(a), img)
        if reference is None:
            continue
        b = reference.qencode(img)
        assert a == b, img.shape
        if k < len(cases) - 1:
            assert np.array_equal(reference.qdecode(a), img) and np.array_equal(oracle.qdecode(b), img)


def _q_model(oracle, img):
    h, w = img.shape
    n = h * w
    u8p, u16p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
    px0 = np.empty(n, np.uint8); adr = np.empty(n, np.uint16); qd = np.empty(n, np.uint8); y = np.empty(n, np.uint8)
    hist = np.zeros(12 * 256, np.uint32)
    oracle.lib.orc_q_model(img.ctypes.data_as(u8p), h, w, px0.ctypes.data_as(u8p), adr.ctypes.data_as(u16p), qd.ctypes.data_as(u8p),
                           y.ctypes.data_as(u8p), hist.ctypes.data_as(C.POINTER(C.c_uint32)))
    return px0, adr, qd, y, hist


def test_q_context_stage_on_arrays_equals_the_raster_model(oracle, golden):
    """orc_q_s2 -- the context stage replayed one context at a time over arrays, the chain kernels' expected output
    (tests/test_chain_kernels.py) -- gives orc_q_model's symbols on every random case and every small golden image, and
    the histogram of (level, symbol) pairs it leads to gives the golden / stored stream through orc_q_entropy_stage."""
    import chain_inputs
    _, streams = golden
    _, stored = inputs.fixtures()
    cases = [(img, stored[f"q_case_{k}"].tobytes()) for k, img in enumerate(inputs.random_q_cases())]
    cases += [(inputs.make(c, h, w), streams[f"q_{c}_{h}x{w}"].tobytes()) for (h, w) in inputs.SMALL_SHAPES for c in inputs.CONTENTS]
    u8p = C.POINTER(C.c_uint8)
    oracle.lib.orc_q_entropy_stage.restype = C.c_long
    for img, want in cases:
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        px0, adr, qd, y, hist = _q_model(oracle, img)
        got_y, _ = chain_inputs.orc_q_s2(oracle, adr, px0, img.reshape(-1))
        assert np.array_equal(got_y, y), img.shape
        assert np.array_equal(qd, adr >> 8), img.shape
        pairs = np.bincount(qd.astype(np.int64) * 256 + got_y, minlength=12 * 256).astype(np.uint32)
        assert np.array_equal(pairs, hist), img.shape
        out = np.empty(2 * h * w + 4096, np.uint16)
        words = oracle.lib.orc_q_entropy_stage(out.ctypes.data_as(C.POINTER(C.c_uint16)), h, w, qd.ctypes.data_as(u8p), got_y.ctypes.data_as(u8p),
                                               pairs.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert out[:words].tobytes() == want, img.shape
