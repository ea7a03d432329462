"""CPU suite: the host side of the batch index build.  nblic_amd_index_build_plan is the one place that lays out the decode
launches of a call and says behind which of them every entry is captured (nblic_amd_index_build_batch builds its launches
from it and from nothing else), so it is checked here against a plain replay: a job advances min(rows, next entry - row)
per launch.  The whole-call refusals need no device either."""
import ctypes as C

import numpy as np
import pytest

CLASSES = [(0, 1), (0, 2), (0, 3), (1, 0)]          # (kind, effort): NBLIC -e1 .. -e3, QNBLIC


def _rows(kind, effort, h, w, serial_rows):
    """serial_rows_per_launch (serial_engine.h); QNBLIC is budgeted as effort 1."""
    if serial_rows > 0:
        return min(serial_rows, h)
    budget = (1 << 22) // (8 if (kind == 0 and effort == 3) else 4 if (kind == 0 and effort == 2) else 1)
    return min(max(budget // w, 1), h)


def _replay(images, serial_rows):
    """(launches per class, {(image, row): launch}) by stepping every job launch by launch."""
    launches, where = {}, {}
    for k, (kind, effort, h, w, R) in enumerate(images):
        rows, count = _rows(kind, effort, h, w, serial_rows), (h - 1) // R
        row, launch = 0, 0
        while row < h:
            nxt = (row // R + 1) * R
            stop = nxt if nxt <= count * R else h
            row += min(rows, stop - row)
            if row < h and row % R == 0:
                where[(k, row)] = launch
            launch += 1
        cls = kind * 4 + effort
        launches[cls] = max(launches.get(cls, 0), launch)
    return launches, where


def _check(pkg, images, serial_rows=0):
    launches, entries = pkg.index_build_plan(images, serial_rows)
    want_launches, where = _replay(images, serial_rows)
    assert launches == want_launches, (images, serial_rows)
    assert len(entries) == len(where) == sum((h - 1) // R for _, _, h, _, R in images)
    got = {(e["image"], e["row"]): e["launch"] for e in entries}
    assert got == where, (images, serial_rows)
    for e in entries:
        kind, effort = images[e["image"]][:2]
        assert e["cls"] == kind * 4 + effort and 0 <= e["launch"] < launches[e["cls"]]
    keys = [(e["cls"], e["launch"]) for e in entries]
    assert keys == sorted(keys), "entries are listed class by class and, within a class, by launch"
    for a, b in zip(entries, entries[1:]):                   # within one capture launch: the caller's order, an image's rows rising
        if (a["cls"], a["launch"]) == (b["cls"], b["launch"]):
            assert (a["image"], a["row"]) < (b["image"], b["row"])


def test_every_row_an_entry(pkg):
    _check(pkg, [(0, 1, 23, 149, 1)])
    _check(pkg, [(0, 1, 23, 149, 1)], 5)
    _check(pkg, [(1, 0, 2, 1, 1)])


def test_spacing_and_rows_that_do_not_divide_each_other(pkg):
    for R, rows in ((7, 3), (3, 7), (6, 4), (4, 6), (5, 5), (10, 3), (3, 10)):
        for h in (R + 1, 40, 67):
            _check(pkg, [(0, 2, h, 150, R)], rows)
    # the automatic rows: 2^22 / 30000 = 139 rows of -e1, 17 of -e3
    _check(pkg, [(0, 1, 1000, 30000, 100), (0, 3, 200, 30000, 9), (0, 1, 1000, 30000, 200)])


def test_one_entry_in_front_of_the_last_row(pkg):
    for h in (2, 3, 40, 65535):
        _check(pkg, [(0, 1, h, 3, h - 1)])
        _check(pkg, [(0, 1, h, 3, h - 1)], 1 if h < 100 else 4096)


def test_mixed_classes(pkg):
    rng = np.random.default_rng(15)
    for _ in range(60):
        images = []
        for _ in range(int(rng.integers(1, 14))):
            kind, effort = CLASSES[int(rng.integers(len(CLASSES)))]
            h = int(rng.integers(2, 80))
            images.append((kind, effort, h, int(rng.integers(1, 300)), int(rng.integers(1, h))))
        for serial_rows in (0, 1, 5, 1000):
            _check(pkg, images, serial_rows)


def test_serial_rows_one(pkg):
    images = [(0, 1, 23, 149, 3), (0, 1, 67, 150, 7), (1, 0, 40, 131, 39), (0, 3, 12, 9, 4)]
    _check(pkg, images, 1)
    launches, entries = pkg.index_build_plan(images, 1)
    assert launches == {1: 67, 4: 40, 3: 12}                 # a row per launch: the tallest image of the class
    assert all(e["launch"] == e["row"] - 1 for e in entries)


def test_fields_out_of_range(pkg):
    good = (0, 1, 23, 149, 3)
    for bad in ((0, 1, 23, 149, 0), (0, 1, 23, 149, 23), (0, 1, 23, 149, -1), (0, 0, 23, 149, 3), (0, 4, 23, 149, 3), (1, 1, 23, 149, 3),
                (2, 1, 23, 149, 3), (0, 1, 0, 149, 3), (0, 1, 23, 0, 3), (0, 1, 65536, 149, 3), (0, 1, 23, 65536, 3), (0, 1, 1, 149, 1)):
        for images in ([bad], [good, bad], [bad, good]):
            with pytest.raises(ValueError):
                pkg.index_build_plan(images)
    with pytest.raises(ValueError):
        pkg.index_build_plan([good], -1)
    lib = pkg.load_library()
    one = (C.c_int * 1)(1)
    assert lib.nblic_amd_index_build_plan(0, one, one, one, one, one, 0, None, None, 0) == -1
    assert lib.nblic_amd_index_build_plan(1, None, one, one, one, one, 0, None, None, 0) == -1
    # the count alone, and a capacity that does not suffice: nothing is written
    cols = [(C.c_int * 1)(v) for v in good]
    entries = (C.c_int * 8)(*([-7] * 8))
    assert lib.nblic_amd_index_build_plan(1, *cols, 0, None, entries, 6) == 7
    assert list(entries) == [-7] * 8


def test_whole_call_refusals_need_no_device(pkg):
    lib = pkg.load_library()
    s = np.zeros(64, np.uint8)
    vp = (C.c_void_p * 1)(s.ctypes.data)
    sz = (C.c_size_t * 1)(64)
    ints = [(C.c_int * 1)(-7) for _ in range(6)]
    lens = (C.c_long * 1)(-7)
    # no context: -1 whatever else is given, status untouched
    assert lib.nblic_amd_index_build_batch(None, 1, vp, sz, ints[0], vp, sz, lens, None, None, *ints[1:]) == -1
    assert ints[5][0] == -7 and lens[0] == -7
    assert lib.nblic_amd_index_build_split(None, None) == -1
    end = C.c_int(-7)
    assert lib.nblic_amd_debug_index_capture(None, 0, 1, 8, 1, 0, None, 0, None, 0, None, 0, 0, None, 0, C.byref(end)) == -1
