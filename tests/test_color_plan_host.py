"""CPU suite: the colour plan without a GPU.  The cost kernel's tile walk on the host (csrc/color_plan.h color_cost_host)
against the whole-array numpy restatement, exact, at the shapes where the walk can go wrong, in all four formats and
three layouts; the choice rule on hand-made cost tables -- every mode, the tie orders, the margin's boundary -- and on the
four constructed classes of frames; the mode helpers; and rct_forward / rct_inverse in every mode."""
import numpy as np
import pytest

import color_plan_inputs as ci
from rct_inputs import exhaustive_frame


@pytest.fixture(scope="module")
def tasks(pkg):
    return ci.cost_tasks(pkg)


def _host(pkg, t, info=None):
    return pkg.color_cost_host(t["raws"], t["rows"], t["cols"], t["fmt"], t["pitches"], t["steps"], t["scale"], t["bias"], info=info)


def test_task_list_covers_the_shapes_formats_and_layouts(tasks):
    assert {(t["rows"], t["cols"]) for t in tasks} == set(ci.SHAPES) | {(256, 256)}
    assert {(t["fmt"], t["layout"]) for t in tasks} == {(f, l) for f in range(4) for l in ci.LAYOUTS}
    assert any(t["scale"] != 1.0 for t in tasks) and any(t["bias"] != 0.0 for t in tasks)


def test_host_walk_equals_the_numpy_restatement(pkg, tasks):
    for k, t in enumerate(tasks):
        info = {}
        got = _host(pkg, t, info)
        assert info["tiles"] == -(-t["rows"] // ci.TILE) * -(-t["cols"] // ci.TILE), k
        want = pkg.color_cost_numpy(*t["planes"])
        assert got.dtype == np.uint64 and np.array_equal(got, want), (k, t["rows"], t["cols"], t["fmt"], t["layout"], got, want)


def test_numpy_restatement_by_hand(pkg):
    """Small planes worked out by hand: the restatement is itself what the walk is compared with."""
    z = np.zeros((1, 1), np.uint8)
    # a single pixel 0: e = -128, |e| = 128, bitlen 8 -> 17; the differences are 128: e = 0 -> 1
    assert pkg.color_cost_numpy(z, z, z).tolist() == [17, 17, 17, 1, 1, 1, 1, 1, 1]
    p = np.array([[128, 130], [131, 120]], np.uint8)
    # (0,0): pred 128, e 0 -> 1; (0,1): pred W 128, e 2 -> 5; (1,0): pred N 128, e 3 -> 5; (1,1): W 131, N 130, NW 128 <= min -> max 131, e -11 -> 9
    assert int(pkg.color_cost_numpy(p, z + np.zeros_like(p), p)[0]) == 1 + 5 + 5 + 9
    # MED's three branches at (1, 1): NW >= max -> min; NW <= min -> max; otherwise W + N - NW
    for w, n, nw, pred in ((10, 20, 30, 10), (10, 20, 5, 20), (10, 20, 15, 15), (20, 10, 20, 10), (7, 7, 7, 7)):
        q = np.array([[nw, n], [w, pred]], np.uint8)
        rest = int(pkg.color_cost_numpy(np.array([[nw, n], [w, pred + 1]], np.uint8), q, q)[0]) - int(pkg.color_cost_numpy(q, q, q)[0])
        assert rest == 2, (w, n, nw)                             # e = 0 costs 1, e = 1 costs 3


def test_refusals(pkg):
    r, g, b = (np.zeros((4, 8), np.uint8) for _ in range(3))
    assert pkg.color_cost_host([r, g, b], 4, 8, 0).tolist() == pkg.color_cost_numpy(r, g, b).tolist()
    for kw in (dict(caps=[32, 31, 32]), dict(pitches=[8, 8, 9]), dict(steps=[1, 0, 1]), dict(scale=2.0), dict(bias=float("nan"))):
        with pytest.raises(ValueError):
            pkg.color_cost_host([r, g, b], 4, 8, 0, **kw)
    for rows, cols in ((0, 8), (4, 0), (65536, 1)):
        with pytest.raises(ValueError):
            pkg.color_cost_host([r, g, b], rows, cols, 0)
    with pytest.raises(ValueError):
        pkg.color_cost_host([r, g, b], 4, 8, 4)
    f = np.zeros((4, 8), np.float16)
    with pytest.raises(ValueError):                               # an element at an odd address
        pkg.color_cost_host([f, f, np.zeros(4 * 8 * 2 + 1, np.uint8)], 4, 8, 1, offsets=(0, 0, 1))


def test_mode_helpers(pkg):
    valid = {0} | {b | d for b in range(3) for d in (4, 8, 12)}
    assert set(pkg.COLOR_MODES) == valid and len(pkg.COLOR_MODES) == 10
    assert pkg.COLOR_PLAIN == 0 and pkg.COLOR_RCT == 0x0D
    for m in range(-1, 257):
        assert pkg.color_mode_valid(m) == (m in valid), m
    for m in valid:
        b = m & 3
        others = [c for c in range(3) if c != b]
        want = [None] * 3
        if m & 4:
            want[others[0]] = b
        if m & 8:
            want[others[1]] = b
        assert [pkg.color_mode_ref(m, c) for c in range(3)] == want, m
    assert [pkg.color_mode_ref(0x0D, c) for c in range(3)] == [1, None, 1]
    for m, c in ((1, 0), (3, 0), (0xFF, 1), (0x0D, 3), (0x0D, -1)):
        with pytest.raises(ValueError):
            pkg.color_mode_ref(m, c)


def _table(plain, diffs):
    """Nine costs: plain[3], and diffs {(c, b): cost of c - b}; every other difference is dear."""
    order = ((0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1))
    return list(plain) + [diffs.get(p, 2 * max(plain)) for p in order]


def test_choose_every_mode(pkg):
    for m in pkg.COLOR_MODES:
        b = m & 3
        others = [c for c in range(3) if c != b]
        diffs = {}
        if m & 4:
            diffs[(others[0], b)] = 100
        if m & 8:
            diffs[(others[1], b)] = 100
        assert pkg.color_choose(_table((1000, 1000, 1000), diffs)) == m, hex(m)
    with pytest.raises(ValueError):
        pkg.color_choose([1] * 8)


def test_choose_ties_go_to_g_then_r_then_b(pkg):
    every = {(c, b): 100 for c in range(3) for b in range(3) if c != b}
    assert pkg.color_choose(_table((1000,) * 3, every)) == 0x0D                                     # all three bases tie: G
    assert pkg.color_choose(_table((1000,) * 3, {k: v for k, v in every.items() if k[1] != 1})) == 0x0C       # R and B tie: R (base 0, both)
    assert pkg.color_choose(_table((1000,) * 3, {k: v for k, v in every.items() if k[1] != 0})) == 0x0D       # G and B tie: G
    assert pkg.color_choose(_table((1000,) * 3, {k: v for k, v in every.items() if k[1] == 2})) == 0x0E       # B alone
    # a smaller total beats the order
    assert pkg.color_choose(_table((1000,) * 3, {**every, (0, 2): 99})) == 0x0E
    # no base has a difference: plain, whatever the plain costs are
    assert pkg.color_choose(_table((5, 1000, 7), {})) == 0


def test_choose_margin_boundary(pkg):
    """64 d == 63 p stays plain; one less takes the difference."""
    p = 64 * 1000
    d = 63 * 1000
    assert 64 * d == 63 * p
    assert pkg.color_choose(_table((p, p, p), {(0, 1): d})) == 0
    assert pkg.color_choose(_table((p, p, p), {(0, 1): d - 1})) == 0x05
    assert pkg.color_choose(_table((p, p, p), {(2, 1): d - 1, (0, 1): d})) == 0x09
    big = 1 << 54                                                # the products do not fit 64 bits
    assert pkg.color_choose(_table((64 * big, 64 * big, 64 * big), {(0, 1): 63 * big})) == 0
    assert pkg.color_choose(_table((64 * big, 64 * big, 64 * big), {(0, 1): 63 * big - 1})) == 0x05


def test_constructed_classes(pkg):
    h, w = 48, 80
    frames = ci.class_frames(h, w)
    costs = [pkg.color_cost_numpy(*fr).astype(np.int64) for fr in frames]
    raws = lambda fr: [np.ascontiguousarray(p) for p in fr]
    for fr, c in zip(frames, costs):
        assert np.array_equal(pkg.color_cost_host(raws(fr), h, w, 0).astype(np.int64), c)
    ci.check_class_modes(pkg, [pkg.color_choose(c) for c in costs])
    c = costs[0]                                                 # the shared class: any base would do
    totals = [c[1] + c[3] + c[8], c[0] + c[5] + c[7], c[2] + c[4] + c[6]]
    assert max(totals) - min(totals) <= 0.003 * min(totals), totals
    assert np.array_equal(frames[3][0], frames[3][1]) and np.array_equal(frames[3][0], frames[3][2])


def test_forward_then_inverse_is_the_identity_in_every_mode(pkg):
    r, g, b = exhaustive_frame()
    for m in pkg.COLOR_MODES:
        t = pkg.rct_forward(r, g, b, mode=m)
        for c in range(3):
            ref = pkg.color_mode_ref(m, c)
            want = (r, g, b)[c] if ref is None else (((r, g, b)[c].astype(np.int16) - (r, g, b)[ref] + 128) % 256).astype(np.uint8)
            assert np.array_equal(t[c], want), (hex(m), c)
        back = pkg.rct_inverse(*t, mode=m)
        assert all(np.array_equal(x, y) for x, y in zip(back, (r, g, b))), hex(m)
    assert all(np.array_equal(x, y) for x, y in zip(pkg.rct_forward(r, g, b), pkg.rct_forward(r, g, b, mode=pkg.COLOR_RCT)))
    with pytest.raises(ValueError):
        pkg.rct_forward(r, g, b, mode=1)
