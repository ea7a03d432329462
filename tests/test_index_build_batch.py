"""GPU suite (-m gpu): the batch index build (nblic_amd_index_build_batch) and its capture kernel.  Many streams go into ONE
call -- modes, widths and R all mixed -- and every index must equal, byte for byte, what nblic_amd_index_build writes for
that stream alone; every plane the oracle's reconstruction; an image that fails fails alone.  k_index_capture is also run
on caller-made bytes (nblic_amd_debug_index_capture): a record no decoder leaves, the plane at every residue mod 4."""
import ctypes as C
import struct
import threading

import numpy as np
import pytest

import inputs
from test_indexed_batch_decode import GEOMS, RANK_AT, REC_BYTES, SYM_AT, _b_bytes, _live, _made
from test_seek_index import CASES, _split, _stream

pytestmark = pytest.mark.gpu

KIND = {"n": 0, "q": 1}
RS = (1, 3, 7)

_cache = {}


def _mixed(gpu_ctx, oracle):
    """[(stream, build_index(stream, R), reconstruction, case)]: every mode x GEOMS x RS, made once per session."""
    if "mixed" not in _cache:
        _cache["mixed"] = [_made(gpu_ctx, oracle, kind, near, effort, h, w, R) + ((kind, near, effort, h, w, R),)
                           for kind, near, effort in CASES for h, w in GEOMS for R in RS]
    return _cache["mixed"]


def _call(gpu_ctx, pkg, streams, every, geoms, planes=True, slack=40, icaps=None, pcaps=None):
    """The C entry with every output buffer `slack` bytes longer than needed and filled with 0x5A.  geoms: (kind, effort, h,
    w) per stream, the geometry its buffers are sized for.  Returns (rc, status, index_lens, indexes, planes, index sizes,
    plane sizes)."""
    n = len(streams)
    ss = [np.frombuffer(s, np.uint8) for s in streams]
    need = [max(pkg.index_bytes(KIND[k], h, w, e, R if 1 <= R < h else 1), 0) for (k, e, h, w), R in zip(geoms, every)]
    px = [h * w for _, _, h, w in geoms]
    xs = [np.full(b + slack, 0x5A, np.uint8) for b in need]
    ps = [np.full(b + slack, 0x5A, np.uint8) for b in px]
    vp = lambda arrs: (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    sz = lambda vals: (C.c_size_t * n)(*vals)
    ints = [(C.c_int * n)(*([-7] * n)) for _ in range(5)]
    lens = (C.c_long * n)(*([-7] * n))
    rc = gpu_ctx.lib.nblic_amd_index_build_batch(gpu_ctx.handle, n, vp(ss), sz([a.size for a in ss]), (C.c_int * n)(*every), vp(xs),
                                                 sz(need if icaps is None else icaps), lens, vp(ps) if planes else None,
                                                 sz(px if pcaps is None else pcaps) if planes else None, *ints)
    return rc, list(ints[4]), list(lens), xs, ps, need, px


def test_mixed_batch_equals_build_index(gpu_ctx, pkg, oracle):
    """All modes, three geometries (odd widths, w = 2 mod 4) and three R in ONE call, planes wanted."""
    made = _mixed(gpu_ctx, oracle)
    before = gpu_ctx.serial_launches()
    with _live(pkg):
        info = {}
        indexes, planes = gpu_ctx.build_index_batch([m[0] for m in made], [m[3][5] for m in made], planes=True, info=info)
    assert info["rc"] == 0 and info["status"] == [0] * len(made)
    assert gpu_ctx.serial_launches() > before
    for (s, ix, rec, case), got, plane in zip(made, indexes, planes):
        assert got is not None and len(got) == len(ix), case
        assert got == ix, case
        assert plane is not None and np.array_equal(plane, rec), case
    assert info["heights"] == [m[3][3] for m in made] and info["widths"] == [m[3][4] for m in made]
    assert info["nears"] == [m[3][1] for m in made] and info["efforts"] == [m[3][2] for m in made]
    split = gpu_ctx.index_build_split()
    assert all(v >= 0 for v in split.values()) and split["launches"] > 0
    _cache["mixed_indexes"] = indexes
    # the C entry, 40 bytes of slack behind every buffer
    with _live(pkg):
        rc, status, lens, xs, ps, need, px = _call(gpu_ctx, pkg, [m[0] for m in made], [m[3][5] for m in made],
                                                   [(m[3][0], m[3][2], m[3][3], m[3][4]) for m in made])
    assert rc == 0 and status == [0] * len(made) and lens == need
    for (s, ix, rec, case), x, p, nb, pb in zip(made, xs, ps, need, px):
        assert x[:nb].tobytes() == ix and (x[nb:] == 0x5A).all(), case
        assert np.array_equal(p[:pb], rec.reshape(-1)) and (p[pb:] == 0x5A).all(), case
    # no planes wanted, and planes wanted for some: the same indexes
    assert gpu_ctx.build_index_batch([m[0] for m in made[:7]], [m[3][5] for m in made[:7]]) == [m[1] for m in made[:7]]


def test_rows_per_launch_do_not_show(gpu_ctx, pkg, oracle):
    """One row and five rows per launch: a job stops and resumes inside its segments, and between them, at other places."""
    made = _mixed(gpu_ctx, oracle)
    try:
        for rows in (1, 5):
            gpu_ctx.set_serial_rows(rows)
            indexes, planes = gpu_ctx.build_index_batch([m[0] for m in made], [m[3][5] for m in made], planes=True)
            for (s, ix, rec, case), got, plane in zip(made, indexes, planes):
                assert got == ix, (rows, case)
                assert np.array_equal(plane, rec), (rows, case)
    finally:
        gpu_ctx.set_serial_rows(0)


def test_lean_image(gpu_ctx, pkg, oracle):
    """300 -e1 streams of one call: more than the lean decoder's threshold.  The lean decoder never writes the symbol ->
    rank bytes back, so a capture that copied them would write entries nblic_amd_index_check refuses."""
    rng = np.random.default_rng(15)
    streams, every = [], []
    for k in range(300):
        h, w = int(rng.integers(5, 13)), int(rng.integers(9, 21))
        streams.append(oracle.encode(inputs.syn1(h, w, 100 + k), 0, 1)[0])
        every.append(int(rng.integers(1, 5)))
    assert pkg.serial_plan(True, 1, 300, 20) & 2, "300 jobs of a launch take the lean image"
    with _live(pkg):
        indexes = gpu_ctx.build_index_batch(streams, every)
    for k, (s, R, ix) in enumerate(zip(streams, every, indexes)):
        assert ix is not None, k
        assert ix == gpu_ctx.build_index(s, R), (k, R)
        assert pkg.check_index(ix, s), k


def _record(rng, kind, row):
    """A record no decoder leaves: arbitrary tables, per re-mapper a permutation in the rank -> symbol bytes, noise in the
    symbol -> rank bytes and in avail / final_ / pad.  Returns (record, the body's record as the kernel must write it)."""
    rec = rng.integers(0, 256, REC_BYTES[kind], dtype=np.uint8)
    rec[0:8] = np.frombuffer(struct.pack("<ii", row, 0), np.uint8)       # next_row, status kRunning
    want = rec.copy()
    want[32:64] = 0                                                      # avail, final_, pad
    if kind == "n":
        sym = np.stack([rng.permutation(20) for _ in range(512)]).astype(np.uint8)
        rec[SYM_AT:SYM_AT + 10240] = sym.reshape(-1)
        want[SYM_AT:SYM_AT + 10240] = sym.reshape(-1)
        want[RANK_AT:SYM_AT] = np.argsort(sym, axis=1).astype(np.uint8).reshape(-1)     # rank[m][sym[m][i]] = i
    return rec, want


CAPTURE_CASES = [("n", 1, 149), ("n", 2, 150), ("n", 3, 151), ("n", 1, 8), ("q", 0, 149)]


@pytest.mark.parametrize("kind,effort,w", CAPTURE_CASES)
def test_capture_on_caller_made_bytes(gpu_ctx, pkg, kind, effort, w):
    rng = np.random.default_rng(1500 + w + effort)
    bb = _b_bytes(kind, effort, w)
    residues = set()
    for offset in (0, 1, 2, 3, 13, 4096):
        for row, next_end in ((1, 2), (2, 0), (40, 47)):
            rec, want = _record(rng, kind, row)
            b = rng.standard_normal(bb // 8).view(np.uint8) if bb else None
            n = min(row, 2)
            rows = rng.integers(0, 256, n * w, dtype=np.uint8)
            residues.add(offset % 4)
            body, end = gpu_ctx.debug_index_capture(KIND[kind], effort, w, row, next_end, rec, b, rows, offset)
            assert body.size == REC_BYTES[kind] + bb + 2 * w
            assert np.array_equal(body[:REC_BYTES[kind]], want), (offset, row, np.flatnonzero(body[:REC_BYTES[kind]] != want)[:8])
            if bb:
                assert np.array_equal(body[REC_BYTES[kind]:REC_BYTES[kind] + bb], b), (offset, row)
            slot = body[REC_BYTES[kind] + bb:]
            assert not slot[:(2 - n) * w].any() and np.array_equal(slot[(2 - n) * w:], rows), (offset, row)
            assert end == next_end, (offset, row)
    assert residues == {0, 1, 2, 3}
    # a record that stands somewhere else, or does not run: nothing is written, and the job keeps its end_row
    for field, value in ((0, 41), (0, 39), (0, 0), (4, 1), (4, -1), (4, 2)):
        rec, _ = _record(rng, kind, 40)
        rec[field:field + 4] = np.frombuffer(struct.pack("<i", value), np.uint8)
        b = rng.standard_normal(bb // 8).view(np.uint8) if bb else None
        body, end = gpu_ctx.debug_index_capture(KIND[kind], effort, w, 40, 47, rec, b, rng.integers(0, 256, 2 * w, dtype=np.uint8), 2)
        assert (body == 0xA7).all() and end == 40, (field, value)


def test_capture_refusals(gpu_ctx, pkg):
    rng = np.random.default_rng(3)
    w, bb = 150, 512 * 150
    rec, _ = _record(rng, "n", 40)
    b, rows = np.zeros(bb, np.uint8), np.zeros(2 * w, np.uint8)
    live = pkg.live_resources()
    good = dict(kind=0, effort=2, w=w, row=40, next_end=47, record=rec, b=b, rows=rows, plane_offset=0)
    for change in (dict(kind=2), dict(kind=1), dict(effort=0), dict(effort=4), dict(w=0), dict(w=65536), dict(row=0), dict(row=65536), dict(next_end=-1),
                   dict(record=rec[:-1]), dict(record=None), dict(b=b[:-8]), dict(b=None), dict(rows=rows[:-1]), dict(rows=rows[:w]), dict(rows=None),
                   dict(plane_offset=4097), dict(row=1)):                # row 1 has one row above, not two
        with pytest.raises(ValueError):
            gpu_ctx.debug_index_capture(**{**good, **change})
    assert pkg.live_resources() == live
    body, end = gpu_ctx.debug_index_capture(**good)
    assert end == 47 and pkg.live_resources() == live


def test_an_image_fails_alone(gpu_ctx, pkg, oracle):
    h, w, R = 40, 131, 6
    s, ix, rec = _made(gpu_ctx, oracle, "n", 0, 2, h, w, R, 7)
    s1, ix1, rec1 = _made(gpu_ctx, oracle, "n", 0, 1, 23, 149, 3)
    e1s, e1ix, _ = _made(gpu_ctx, oracle, "n", 0, 1, h, w, R, 7)
    g_bad, g_good = ("n", 2, h, w), ("n", 1, 23, 149)
    forged = b"NBLIC0.4" + s[8:]
    need = pkg.index_bytes(0, h, w, 2, R)
    # (stream, R, geometry, index cap or None, does it reach the device)
    bads = [(s[:len(s) // 3], R, g_bad, None, True), (e1s[:len(e1s) // 3], R, ("n", 1, h, w), None, True), (forged, R, g_bad, None, False),
            (s, 0, g_bad, None, False), (s, h, g_bad, None, False), (s, R, g_bad, need - 1, False)]
    with _live(pkg):
        for bad, bad_R, geom, cap, launched in bads:
            for at in (0, 1, 2):
                streams, every, geoms = [s1, s1], [3, 3], [g_good, g_good]
                streams.insert(at, bad); every.insert(at, bad_R); geoms.insert(at, geom)
                icaps = None
                if cap is not None:
                    icaps = [pkg.index_bytes(0, 23, 149, 1, 3)] * 3
                    icaps[at] = cap
                rc, status, lens, xs, ps, sizes, px = _call(gpu_ctx, pkg, streams, every, geoms, icaps=icaps)
                assert rc == -1 and status == [-1 if k == at else 0 for k in range(3)], (at, bad_R, cap, status)
                assert lens == [-1 if k == at else len(ix1) for k in range(3)]
                if launched:                                             # decoded and found short: zeroed, the slack untouched
                    assert not xs[at][:sizes[at]].any() and (xs[at][sizes[at]:] == 0x5A).all()
                    assert not ps[at][:px[at]].any() and (ps[at][px[at]:] == 0x5A).all()
                else:
                    assert (xs[at] == 0x5A).all() and (ps[at] == 0x5A).all(), "a refused image's buffer was written"
                for k in range(3):
                    if k != at:
                        assert xs[k][:sizes[k]].tobytes() == ix1 and (xs[k][sizes[k]:] == 0x5A).all()
                        assert np.array_equal(ps[k][:px[k]], rec1.reshape(-1)) and (ps[k][px[k]:] == 0x5A).all()
        # a plane buffer one byte short
        rc, status, lens, xs, ps, sizes, px = _call(gpu_ctx, pkg, [s1, s, s1], [3, R, 3], [g_good, g_bad, g_good], pcaps=[23 * 149, h * w - 1, 23 * 149])
        assert rc == -1 and status == [0, -1, 0] and lens[1] == -1 and (xs[1] == 0x5A).all() and (ps[1] == 0x5A).all()
        # nothing but refused images: no kernel is launched
        before = gpu_ctx.serial_launches()
        live = pkg.live_resources()
        rc, status, lens, *_ = _call(gpu_ctx, pkg, [forged, s, s], [R, 0, R], [g_bad] * 3, icaps=[need, need, 5])
        assert rc == -1 and status == [-1, -1, -1] and lens == [-1, -1, -1]
        assert gpu_ctx.serial_launches() == before, "a call of refused images launched a kernel"
        assert pkg.live_resources() == live
    # the Python entry: None for the failed image, the header fields of every stream that parsed
    info = {}
    got = gpu_ctx.build_index_batch([s1, s[:len(s) // 3], forged, s], [3, R, R, R], info=info)
    assert got == [ix1, None, None, ix] and info["rc"] == -1 and info["status"] == [0, -1, -1, 0]
    assert info["heights"] == [23, h, 0, h] and info["efforts"] == [1, 2, 0, 2]


def test_round_trip_through_the_indexed_batch_decode(gpu_ctx, pkg, oracle):
    made = _mixed(gpu_ctx, oracle)
    indexes = _cache.get("mixed_indexes") or gpu_ctx.build_index_batch([m[0] for m in made], [m[3][5] for m in made])
    planes = gpu_ctx.decode_batch_indexed([(m[0], ix) for m, ix in zip(made, indexes)])
    for (s, _, rec, case), plane in zip(made, planes):
        assert plane is not None and np.array_equal(plane, rec), case


def test_foreign_streams(gpu_ctx, pkg, oracle):
    """Streams no encoder here writes -- every (near, k_step) pair of a decoder's range, all efforts -- of the plane
    `checker`, whose hashes tests/golden/foreign_streams.json holds next to those of the planes the reference decoded them to."""
    import hashlib
    plane = inputs.foreign_planes()["checker"]
    cases = inputs.foreign_streams(oracle, plane)
    stored = inputs.foreign_golden()
    for k, effort in enumerate(inputs.FOREIGN_EFFORTS):
        part = cases[140 * k:140 * (k + 1)]
        assert hashlib.sha256(b"".join(c[1] for c in part)).hexdigest() == stored[f"checker_e{effort}"]["streams_sha256"]
    R = 5
    with _live(pkg):
        indexes, planes = gpu_ctx.build_index_batch([c[1] for c in cases], R, planes=True)
    for k, effort in enumerate(inputs.FOREIGN_EFFORTS):
        got = b"".join(p.tobytes() for p in planes[140 * k:140 * (k + 1)])
        assert hashlib.sha256(got).hexdigest() == stored[f"checker_e{effort}"]["planes_sha256"], effort
    for (head, s, rec), ix, p in zip(cases, indexes, planes):
        assert ix is not None and ix == gpu_ctx.build_index(s, R), head
        assert np.array_equal(p, rec), head


def test_next_to_encode_batch(gpu_ctx, pkg, oracle):
    a = _made(gpu_ctx, oracle, "n", 0, 2, 40, 131, 6, 7)
    b = _made(gpu_ctx, oracle, "n", 0, 1, 67, 150, 7)
    imgs = [inputs.syn1(64, 96, 40 + k) for k in range(12)]
    want = [oracle.encode(i, 0, 1)[0] for i in imgs]
    got, errs = [], []

    def build():
        try:
            for _ in range(4):
                got.append(gpu_ctx.build_index_batch([a[0], b[0], a[0]], [6, 7, 6]))
        except Exception as e:                                  # pragma: no cover - reported below
            errs.append(e)

    t = threading.Thread(target=build)
    t.start()
    for _ in range(4):
        assert gpu_ctx.encode_batch(imgs) == want
    t.join()
    assert not errs, errs
    assert got == [[a[1], b[1], a[1]]] * 4
