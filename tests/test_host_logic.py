"""CPU suite: the product's host-compilable model code (csrc/model.h) and the double-carried
least-squares arithmetic (csrc/lsq_f64.h) that the serial GPU kernels use, compiled into a scalar
harness (tests/host_harness.cpp) and checked against the oracle.  No GPU, no product library paths
beyond the host range coder."""
import os

import numpy as np
import pytest

import inputs
import lsq_cases


@pytest.fixture(scope="module")
def harness():
    return lsq_cases.load_harness()


def harness_encode(lib, pkg, img, near, effort):
    """(stream, reconstruction, solves redone with integers, the same split by system)"""
    h, w = img.shape
    coded, rec, fallbacks, by_system, _ = lsq_cases.model_encode(lib, img, near, effort)
    assert fallbacks == sum(by_system)
    k_step = min(max(3 + 2 * near, 3), 16)
    header = b"NBLIC0.3" + bytes([1, h >> 8, h & 255, w >> 8, w & 255, near, k_step, effort])
    return header + pkg.range_code(coded), rec, fallbacks, by_system


def test_divide_free_helpers_exhaustive(harness):
    assert harness.hh_check_divide_free() == 0


def test_symbol_bins_lane_layout_matches_the_walk(harness):
    """The decoders compute a symbol's bin probabilities on the lanes (serial_engine.hip decode_symbol): prefix node t on
    lane t, the suffix tree in heap order.  Every (k_step, level pair, symbol): the nodes the reference's walk visits are
    the ones that layout names."""
    assert harness.hh_check_symbol_lanes() == 0


@pytest.mark.parametrize("qnblic", [0, 1])
def test_lane_table_reproduces_the_model(harness, qnblic):
    """csrc/lane_table.h (one model term per lane: the serial kernels' pixel front) walked on the CPU over random,
    extreme, smooth and flat planes of widths 1..64, rows >= 2: predictor, activity, level, context address and
    regressors equal model.h's on the taps the reference's sampling rules deliver."""
    assert harness.hh_check_lane_front(qnblic, 7) == 0


@pytest.mark.parametrize("near,effort", [(0, 1), (0, 2), (0, 3), (2, 1), (2, 2), (3, 3), (9, 1), (1, 3)])
def test_model_headers_and_f64_least_squares_equal_oracle(harness, pkg, oracle, near, effort):
    for (h, w) in [(17, 13), (64, 64), (5, 300)]:
        for content in inputs.CONTENTS:
            img = inputs.make(content, h, w)
            s, rec, *_ = harness_encode(harness, pkg, img, near, effort)
            ws, wrec, *_ = oracle.encode(img, near, effort)
            assert s == ws and np.array_equal(rec, wrec), (h, w, content)
        for content in inputs.HARD_EDGED:                       # two-level planes: the ones that reach the integer redo
            img = inputs.make_hard(content, h, w)
            s, rec, *_ = harness_encode(harness, pkg, img, near, effort)
            ws, wrec, *_ = oracle.encode(img, near, effort)
            assert s == ws and np.array_equal(rec, wrec), (h, w, content)


def test_f64_least_squares_on_a_photograph_and_noise(harness, pkg, oracle):
    """Kodak crops (the stored 64x96 one; a 128x160 one read in place where the images are) and uniform noise at
    effort 3: the exact-range guard may send pixels to the integer redo, the bytes must not change.  On these inputs it
    sends none (the count is 0 in every case); the hard-edged planes below are the ones where it does -- at least eight
    solves each, all of them system 0 -- and there the bytes must not change either."""
    meta, stored = inputs.fixtures()
    frames = [inputs.noise(96, 96, 3), stored["kodak_crops"][sorted(meta["kodak_crops"]).index("05.bmp")]]
    kodak = os.path.join(inputs.KODAK_DIR, "05.bmp")
    if os.path.exists(kodak):
        frames.append(np.ascontiguousarray(inputs.read_gray_bmp(kodak)[100:228, 200:360]))
    for img in frames:
        for near, effort in [(0, 3), (2, 2)]:
            s, rec, fallbacks, _ = harness_encode(harness, pkg, img, near, effort)
            ws, wrec, *_ = oracle.encode(img, near, effort)
            assert s == ws and np.array_equal(rec, wrec)
            assert fallbacks == 0                                # photographs and noise never reach the redo: hence the planes below
    hard = [("step_v", 64, 64, [(2, 2), (9, 2), (1, 3), (2, 3), (9, 3)]), ("step_v", 33, 57, [(2, 2), (9, 2), (1, 3), (2, 3), (9, 3)]),
            ("stripes_h", 64, 64, [(2, 2), (9, 2)]), ("step_h", 24, 1500, [(2, 2), (9, 2)]), ("stripes_h", 24, 1500, [(2, 2), (9, 2)]),
            ("bars_v", 4, 52000, [(2, 2), (2, 3)]), ("bars_v", 6, 30000, [(2, 2), (2, 3)])]
    for content, h, w, modes in hard:
        img = inputs.make_hard(content, h, w)
        for near, effort in modes:
            s, rec, fallbacks, by_system = harness_encode(harness, pkg, img, near, effort)
            ws, wrec, *_ = oracle.encode(img, near, effort)
            assert s == ws and np.array_equal(rec, wrec), (content, h, w, near, effort)
            assert fallbacks >= 8 and by_system == (fallbacks, 0), (content, h, w, near, effort, fallbacks, by_system)
