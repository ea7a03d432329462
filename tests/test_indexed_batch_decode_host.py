"""CPU suite: the host side of the indexed batch decode.  nblic_amd_indexed_decode_plan is the one place that orders the
segments of a call (nblic_amd_decode_batch_indexed builds its rounds from it and from nothing else), so the ordering rules
are checked here on random mixes; the whole-call refusals need no device either."""
import ctypes as C

import numpy as np
import pytest

CLASSES = [(0, 1), (0, 2), (0, 3), (1, 0)]          # (kind, effort): NBLIC -e1 .. -e3, QNBLIC
CAPS = (1, 2, 3, 7, 0)                              # 0: one round


def _mix(rng):
    n = int(rng.integers(1, 13))
    images, rows = [], []
    for _ in range(n):
        kind, effort = CLASSES[int(rng.integers(len(CLASSES)))]
        h, w = int(rng.integers(2, 60)), int(rng.integers(1, 300))
        R = int(rng.integers(1, h))                  # 1 .. h - 1
        images.append((kind, effort, h, w, R))
        if rng.integers(2):
            rows.append((0, h))
        else:
            r0 = int(rng.integers(0, h))
            rows.append((r0, int(rng.integers(r0 + 1, h + 1))))
    return images, rows


def _check(images, rows, cap, jobs):
    by_image = {}
    for j in jobs:
        by_image.setdefault(j["image"], []).append(j)
    assert sorted(by_image) == list(range(len(images)))
    for k, (kind, effort, h, w, R) in enumerate(images):
        r0, r1 = rows[k]
        mine = by_image[k]
        covered = np.zeros(h, np.int32)
        for j in mine:
            assert j["first_row"] == j["segment"] * R and (j["first_row"] % R == 0 or j["first_row"] == 0)
            end = j["end_row"] if j["end_row"] else h
            assert j["first_row"] < end <= h
            assert (j["end_row"] == 0) == (end == h), "end_row is 0 only for a job that ends at h"
            assert j["cls"] == kind * 4 + effort
            covered[j["first_row"]:end] += 1
        assert (covered[r0:r1] == 1).all(), "every wanted row lies in exactly one job"
        assert covered[:(r0 // R) * R].sum() == 0 and covered[r1:].sum() == 0, "nothing outside the segments of the range"
        assert sorted(j["segment"] for j in mine) == list(range(r0 // R, (r1 - 1) // R + 1))
        order = sorted(mine, key=lambda j: j["segment"])
        rounds = [j["round"] for j in order]
        assert all(a >= b for a, b in zip(rounds, rounds[1:])), "a higher segment never runs in a later round"
    per_round = {}
    for j in jobs:
        per_round.setdefault(j["round"], []).append(j)
    assert sorted(per_round) == list(range(len(per_round)))
    assert [j["round"] for j in jobs] == sorted(j["round"] for j in jobs), "listed round by round"
    for r, js in per_round.items():
        if cap > 0:
            assert len(js) <= cap
        classes = [j["cls"] for j in js]
        runs = [c for i, c in enumerate(classes) if i == 0 or classes[i - 1] != c]
        assert len(runs) == len(set(runs)), "the jobs of a class are neighbours in a round: one launch per class"
    if cap <= 0:
        assert set(per_round) == {0}


def test_plan_properties_on_random_mixes(pkg):
    rng = np.random.default_rng(14)
    for _ in range(60):
        images, rows = _mix(rng)
        for cap in CAPS:
            _check(images, rows, cap, pkg.indexed_decode_plan(images, rows, cap))
        whole = pkg.indexed_decode_plan(images, None, 3)
        _check(images, [(0, im[2]) for im in images], 3, whole)


def test_plan_of_ranges_inside_and_across_a_boundary(pkg):
    h, w, R = 50, 31, 8
    im = [(0, 1, h, w, R)]
    one = pkg.indexed_decode_plan(im, [(17, 23)])
    assert [(j["segment"], j["first_row"], j["end_row"]) for j in one] == [(2, 16, 23)]
    for k in range(1, (h - 1) // R + 1):
        two = pkg.indexed_decode_plan(im, [(k * R - 1, k * R + 1)])
        assert [(j["segment"], j["first_row"], j["end_row"]) for j in two] == [(k, k * R, k * R + 1), (k - 1, (k - 1) * R, k * R)]
        assert len(pkg.indexed_decode_plan(im, [(k * R, k * R + 1)])) == 1
    last = pkg.indexed_decode_plan(im, [(h - 1, h)])
    assert [(j["segment"], j["end_row"]) for j in last] == [((h - 1) // R, 0)]
    three = pkg.indexed_decode_plan(im, [(7, 17)], 2)
    assert [(j["segment"], j["round"]) for j in three] == [(2, 0), (1, 0), (0, 1)]


def test_plan_refuses_fields_out_of_range(pkg):
    good = (0, 1, 20, 30, 4)
    for bad in ((0, 0, 20, 30, 4), (1, 1, 20, 30, 4), (2, 1, 20, 30, 4), (0, 4, 20, 30, 4), (0, 1, 0, 30, 4), (0, 1, 20, 0, 4),
                (0, 1, 20, 30, 0), (0, 1, 70000, 30, 4)):
        with pytest.raises(ValueError):
            pkg.indexed_decode_plan([good, bad])
    for rows in ((0, 0), (5, 5), (6, 3), (-1, 4), (0, 21)):
        with pytest.raises(ValueError):
            pkg.indexed_decode_plan([good], [rows])
    with pytest.raises(ValueError):
        pkg.indexed_decode_plan([])
    lib = pkg.load_library()
    one = (C.c_int * 1)(1)
    assert lib.nblic_amd_indexed_decode_plan(1, one, one, one, one, one, one, None, 0, None, 0) == -1      # exactly one of row0 / row1


def test_whole_call_refusals_leave_status_untouched(pkg):
    lib = pkg.load_library()
    n = 2
    status = (C.c_int * n)(77, 77)
    ints = [(C.c_int * n)() for _ in range(4)]
    buf = np.zeros(64, np.uint8)
    ptrs = (C.c_void_p * n)(buf.ctypes.data, buf.ctypes.data)
    sizes = (C.c_size_t * n)(64, 64)
    rows = (C.c_int * n)(0, 0)
    args = lambda **kw: [kw.get("ctx"), kw.get("n", n), kw.get("streams", ptrs), sizes, kw.get("indexes", ptrs), sizes, kw.get("row0"), kw.get("row1"),
                         kw.get("outs", ptrs), sizes, *ints, status]
    holes = (C.c_void_p * n)(buf.ctypes.data, None)
    for kw in (dict(), dict(n=0), dict(n=-1), dict(streams=None), dict(indexes=None), dict(outs=None), dict(streams=holes), dict(indexes=holes),
               dict(outs=holes), dict(row0=rows), dict(row1=rows)):
        assert lib.nblic_amd_decode_batch_indexed(*args(**kw)) == -1, kw
        assert list(status) == [77, 77], kw
    assert lib.nblic_amd_indexed_decode_split(None, None) == -1
    assert lib.nblic_amd_debug_index_kernels(None, None, 0, 0, 0, 0, 0, None, None, None, None, 0, None, 0, None, 0, None) == -1
