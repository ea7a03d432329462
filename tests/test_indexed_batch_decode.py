"""GPU suite (-m gpu): the indexed batch decode (nblic_amd_decode_batch_indexed) and its two kernels.  Many streams and
their seek indexes go into ONE call -- modes, widths, R and the alignment of the entries all mixed -- and every plane, every
row range must equal the oracle's reconstruction bit for bit; a forged or foreign image fails alone.  The kernels are also
run on caller-made bytes (nblic_amd_debug_index_kernels), the index uploaded at every residue of the address mod 16."""
import ctypes as C
import struct
import threading

import numpy as np
import pytest

import inputs
from test_seek_index import CASES, _join, _reseal_entry, _split, _stream

pytestmark = pytest.mark.gpu

GEOMS = [(23, 149), (67, 150), (40, 131)]
REC_BYTES = {"n": 86080, "q": 12352}
HEAD = 168                                         # the checkpoint head in front of an entry's body
RANK_AT, SYM_AT = 64 + (2048 + 4096 + 512 * 20) * 4, 64 + (2048 + 4096 + 512 * 20) * 4 + 512 * 20   # kRecRank, kRecSym in bytes of the record
COUNTERS_AT = 64 + 2048 * 4

_cache = {}


def _made(gpu_ctx, oracle, kind, near, effort, h, w, R, seed=5):
    """(stream, index, reconstruction), made once per session."""
    key = (kind, near, effort, h, w, seed)
    if key not in _cache:
        _cache[key] = _stream(oracle, kind, near, effort, h, w, seed)
    s, rec = _cache[key]
    if key + (R,) not in _cache:
        _cache[key + (R,)] = gpu_ctx.build_index(s, R)
    return s, _cache[key + (R,)], rec


def _b_bytes(kind, effort, w):
    return (1024 if effort == 3 else 512 if effort == 2 else 0) * w if kind == "n" else 0


def _call(gpu_ctx, pairs, rows=None, slack=40, caps=None):
    """The C entry with every output buffer `slack` bytes longer than needed and filled with 0x5A: (rc, status, outs)."""
    n = len(pairs)
    ss = [np.frombuffer(s, np.uint8) for s, _ in pairs]
    xs = [np.frombuffer(x, np.uint8) for _, x in pairs]
    dims = [struct.unpack_from("<ii", x, 16) for _, x in pairs]
    want = [(h if rows is None else rows[k][1] - rows[k][0]) * w for k, (h, w) in enumerate(dims)]
    outs = [np.full(max(b, 0) + slack, 0x5A, np.uint8) for b in want]
    vp = lambda arrs: (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    sz = lambda vals: (C.c_size_t * n)(*vals)
    ints = [(C.c_int * n)(*([-7] * n)) for _ in range(5)]
    r0 = r1 = None
    if rows is not None:
        r0, r1 = (C.c_int * n)(*[r[0] for r in rows]), (C.c_int * n)(*[r[1] for r in rows])
    rc = gpu_ctx.lib.nblic_amd_decode_batch_indexed(gpu_ctx.handle, n, vp(ss), sz([a.size for a in ss]), vp(xs), sz([a.size for a in xs]), r0, r1,
                                                    vp(outs), sz(want if caps is None else caps), *ints)
    return rc, list(ints[4]), outs, want


class _live:
    """nblic_amd_debug_live must return to what it was before the calls inside."""
    def __init__(self, pkg):
        self.pkg = pkg

    def __enter__(self):
        self.before = self.pkg.live_resources()

    def __exit__(self, *exc):
        if exc[0] is None:
            assert self.pkg.live_resources() == self.before, "the indexed batch decode kept a device resource"


def test_mixed_batch_matches_the_oracle(gpu_ctx, pkg, oracle):
    """All modes, three geometries (odd widths, w = 2 mod 4) and three R in ONE call: classes, widths, R and the residues of
    the entries' addresses all differ inside it."""
    made = [_made(gpu_ctx, oracle, kind, near, effort, h, w, R) + ((kind, near, effort, h, w, R),)
            for kind, near, effort in CASES for h, w in GEOMS for R in (1, 3, 7)]
    singles = [gpu_ctx.decode_indexed(s, ix) for s, ix, _, _ in made]
    before = gpu_ctx.serial_launches()
    with _live(pkg):
        info = {}
        planes = gpu_ctx.decode_batch_indexed([(s, ix) for s, ix, _, _ in made], info=info)
    assert info["rc"] == 0 and info["status"] == [0] * len(made)
    assert gpu_ctx.serial_launches() > before
    for (s, ix, rec, case), plane, single in zip(made, planes, singles):
        assert plane is not None and plane.shape == rec.shape, case
        assert np.array_equal(plane, rec), case                                # the oracle's plane: what the test rests on
        assert np.array_equal(plane, single), case                             # (the same path called with one image)
    split = gpu_ctx.indexed_decode_split()
    assert all(v >= 0 for v in split.values()) and split["rounds"] > 0


def test_row_ranges_in_one_batch(gpu_ctx, pkg, oracle):
    pairs, rows, want = [], [], []
    for kind, near, effort in CASES:
        for (h, w), R in (((67, 150), 7), ((23, 149), 3), ((40, 131), 1)):
            s, ix, rec = _made(gpu_ctx, oracle, kind, near, effort, h, w, R)
            k = ((h - 1) // R) // 2 + 1
            ranges = [(k * R - 1, k * R + 1), (k * R, k * R + 1), (0, 1), (h - 1, h), (1, h - 1), (k * R - R - 1, min(h, k * R + 2))]
            assert (ranges[-1][1] - 1) // R - ranges[-1][0] // R >= 2          # the last one lies across three segments at least
            for r in ranges:
                pairs.append((s, ix)); rows.append(r); want.append(rec[r[0]:r[1]])
    got = gpu_ctx.decode_batch_indexed(pairs, rows)
    for g, wnt, r in zip(got, want, rows):
        assert g is not None and np.array_equal(g, wnt), r
    rc, status, outs, sizes = _call(gpu_ctx, pairs, rows)
    assert rc == 0 and status == [0] * len(pairs)
    for o, b, wnt, r in zip(outs, sizes, want, rows):
        assert np.array_equal(o[:b], wnt.reshape(-1)), r
        assert (o[b:] == 0x5A).all(), ("bytes behind the range were written", r)


def _forge(ix, e, kind, effort, w, what):
    """The index with entry e (1-based) changed in one place and resealed: every check of the entry alone still passes."""
    head, ents = _split(ix)
    b = bytearray(ents[e - 1])
    rec_b, bb = REC_BYTES[kind], _b_bytes(kind, effort, w)
    rows_at = HEAD + rec_b + bb
    if what == "row0":
        b[rows_at + 3] ^= 0x04
    elif what == "row1":
        b[rows_at + w + 17] ^= 0x01
    elif what == "counter":
        at = next(HEAD + COUNTERS_AT + 4 * i for i in range(4096) if struct.unpack_from("<H", b, HEAD + COUNTERS_AT + 4 * i)[0] > 1)
        struct.pack_into("<H", b, at, struct.unpack_from("<H", b, at)[0] - 1)
    elif what == "sym":
        m = 7 * 20                                                       # re-mapper 7: ranks 0 and 1 change places, and the inverse with them
        s0, s1 = b[HEAD + SYM_AT + m], b[HEAD + SYM_AT + m + 1]
        b[HEAD + SYM_AT + m], b[HEAD + SYM_AT + m + 1] = s1, s0
        b[HEAD + RANK_AT + m + s1], b[HEAD + RANK_AT + m + s0] = 0, 1
    elif what == "B":
        at = HEAD + rec_b + 8 * 1000
        v = struct.unpack_from("<d", b, at)[0]
        struct.pack_into("<d", b, at, v + 1.0)
    else:
        raise AssertionError(what)
    assert bytes(b) != ents[e - 1], what
    return _join(head, ents[:e - 1] + [_reseal_entry(bytes(b))] + ents[e:])


def test_rounds_and_forged_entries(gpu_ctx, pkg, oracle):
    """Three 67 x 150 images at R = 7 (30 segments) in rounds of 2 and of 3.  Image 1's index has one resealed entry that does
    not follow from the segment in front of it -- at a boundary whose two segments run in different rounds, and at one
    inside a round: image 1 fails alone and leaves no pixel."""
    h, w, R = 67, 150, 7
    e1 = [_made(gpu_ctx, oracle, "n", 0, 1, h, w, R, seed) for seed in (5, 6, 7)]
    e2 = _made(gpu_ctx, oracle, "n", 0, 2, h, w, R, 6)
    try:
        with _live(pkg):
            for per_round in (2, 3):
                gpu_ctx.set_index_round(per_round)
                planes = gpu_ctx.decode_batch_indexed([(s, ix) for s, ix, _ in e1])
                assert all(np.array_equal(p, rec) for p, (_, _, rec) in zip(planes, e1)), per_round
                for what in ("row0", "row1", "counter", "sym", "B"):
                    mid = e2 if what == "B" else e1[1]
                    trio = [e1[0], mid, e1[2]]
                    plan = pkg.indexed_decode_plan([(0, 2 if t is e2 else 1, h, w, R) for t in trio], None, per_round)
                    rounds = {j["segment"]: j["round"] for j in plan if j["image"] == 1}
                    across = [e for e in range(1, 10) if rounds[e] != rounds[e - 1]]
                    inside = [e for e in range(1, 10) if rounds[e] == rounds[e - 1]]
                    assert across and inside, (per_round, rounds)
                    for e in (across[len(across) // 2], inside[len(inside) // 2]):
                        forged = _forge(mid[1], e, "n", 2 if what == "B" else 1, w, what)
                        assert pkg.check_index(forged, mid[0]), (what, e)
                        rc, status, outs, sizes = _call(gpu_ctx, [(trio[0][0], trio[0][1]), (mid[0], forged), (trio[2][0], trio[2][1])])
                        assert rc == -1 and status == [0, -1, 0], (per_round, what, e, status)
                        assert not outs[1][:sizes[1]].any() and (outs[1][sizes[1]:] == 0x5A).all(), (per_round, what, e)
                        for k in (0, 2):
                            assert np.array_equal(outs[k][:sizes[k]], trio[k][2].reshape(-1)), (per_round, what, e, k)
                # the same images with a true index, one of them -e2: two classes in every round they share
                planes = gpu_ctx.decode_batch_indexed([(e1[0][0], e1[0][1]), (e2[0], e2[1]), (e1[2][0], e1[2][1])])
                assert all(np.array_equal(p, t[2]) for p, t in zip(planes, (e1[0], e2, e1[2]))), per_round
    finally:
        gpu_ctx.set_index_round(0)


def test_lean_image(gpu_ctx, pkg, oracle):
    """900 segments in one call, 300 per class: more than the lean decoder's threshold.  The lean decoder never writes the
    rank -> symbol bytes back, so a chain kernel that compared them would refuse these images and no others."""
    made = [_made(gpu_ctx, oracle, kind, near, effort, 300, 40, 1, 4) for kind, near, effort in (("n", 0, 1), ("n", 2, 2), ("q", 0, 0))]
    assert pkg.serial_plan(True, 1, 300, 40) & 2, "300 jobs of a launch take the lean image"
    planes = gpu_ctx.decode_batch_indexed([(s, ix) for s, ix, _ in made])
    for p, (_, _, rec) in zip(planes, made):
        assert p is not None and np.array_equal(p, rec)


def test_wide_rows_next_to_narrow_ones(gpu_ctx, pkg, oracle):
    """4 x 30000 (taps from memory) and 23 x 149 (rows in LDS), both -e1 at R = 1: one launch."""
    wide = _made(gpu_ctx, oracle, "n", 0, 1, 4, 30000, 1, 3)
    narrow = _made(gpu_ctx, oracle, "n", 0, 1, 23, 149, 1)
    plan = pkg.indexed_decode_plan([(0, 1, 4, 30000, 1), (0, 1, 23, 149, 1)])
    assert {j["round"] for j in plan} == {0} and {j["cls"] for j in plan} == {1}
    planes = gpu_ctx.decode_batch_indexed([(wide[0], wide[1]), (narrow[0], narrow[1])])
    assert np.array_equal(planes[0], wide[2]) and np.array_equal(planes[1], narrow[2])
    rows = gpu_ctx.decode_batch_indexed([(wide[0], wide[1]), (narrow[0], narrow[1])], [(2, 3), (11, 13)])
    assert np.array_equal(rows[0], wide[2][2:3]) and np.array_equal(rows[1], narrow[2][11:13])


def test_pairs_straight_from_the_indexed_batch_encode(gpu_ctx, pkg):
    shapes = [(64, 96), (37, 131), (90, 50), (64, 96), (37, 131), (90, 50), (33, 77), (12, 40)]
    imgs = [inputs.syn1(h, w, 60 + k) for k, (h, w) in enumerate(shapes)]
    every = [5, 16, 5, 16, 5, 16, 5, 16]                                 # 12 x 40 at R = 16: no index
    pairs = gpu_ctx.encode_batch_indexed(imgs, every)
    assert pairs[7][1] is None and all(ix is not None for _, ix in pairs[:7])
    planes = gpu_ctx.decode_batch_indexed(pairs)
    assert planes[7] is None
    for p, img in zip(planes[:7], imgs):
        assert p is not None and np.array_equal(p, img)
    rows = gpu_ctx.decode_batch_indexed(pairs[:7], [(3, h - 2) for h, _ in shapes[:7]])
    for r, img in zip(rows, imgs):
        assert np.array_equal(r, img[3:img.shape[0] - 2])


def test_per_image_refusals(gpu_ctx, pkg, oracle):
    h, w, R = 40, 131, 6
    s, ix, rec = _made(gpu_ctx, oracle, "n", 0, 2, h, w, R, 7)
    other, _, _ = _made(gpu_ctx, oracle, "n", 0, 2, h, w, R, 8)
    s1, ix1, rec1 = _made(gpu_ctx, oracle, "n", 0, 1, 23, 149, 3)
    flipped = bytearray(ix)
    flipped[96 + 8 + 5000] ^= 0x10
    good = (s1, ix1)
    with _live(pkg):
        for bad in ((other, ix), (s, ix[:len(ix) // 2]), (s, ix[:-1]), (s, bytes(flipped)), (s[:-1], ix)):
            for at in (0, 1, 2):
                pairs = [good, good]
                pairs.insert(at, bad)
                rc, status, outs, sizes = _call(gpu_ctx, pairs)
                assert rc == -1 and status == [-1 if k == at else 0 for k in range(3)], (at, status)
                assert (outs[at] == 0x5A).all(), "a refused image's buffer was written"
                for k in range(3):
                    if k != at:
                        assert np.array_equal(outs[k][:sizes[k]], rec1.reshape(-1)) and (outs[k][sizes[k]:] == 0x5A).all()
        # a buffer one byte short, a range that ends behind the image: refused alone
        rc, status, outs, sizes = _call(gpu_ctx, [good, (s, ix), good], caps=[23 * 149, h * w - 1, 23 * 149])
        assert rc == -1 and status == [0, -1, 0] and (outs[1] == 0x5A).all()
        rc, status, outs, sizes = _call(gpu_ctx, [good, (s, ix), good], rows=[(0, 23), (5, h + 1), (2, 4)])
        assert rc == -1 and status == [0, -1, 0] and (outs[1] == 0x5A).all()
        assert np.array_equal(outs[2][:sizes[2]], rec1[2:4].reshape(-1))
        rc, status, outs, sizes = _call(gpu_ctx, [(s, ix), good], rows=[(7, 9), (2, 4)], caps=[2 * w - 1, 2 * 149])
        assert rc == -1 and status == [-1, 0]
        for rows in ([(5, 5)], [(6, 3)], [(-1, 4)]):
            rc, status, outs, _ = _call(gpu_ctx, [(s, ix)], rows=rows, caps=[h * w])
            assert rc == -1 and status == [-1]
        before = gpu_ctx.serial_launches()
        live = pkg.live_resources()
        rc, status, outs, _ = _call(gpu_ctx, [(other, ix), (s, bytes(flipped)), (s, ix)], caps=[h * w, h * w, 5])
        assert rc == -1 and status == [-1, -1, -1]
        assert gpu_ctx.serial_launches() == before, "a call of refused images launched a kernel"
        assert pkg.live_resources() == live
        assert np.array_equal(gpu_ctx.decode_batch_indexed([(s, ix)])[0], rec)


KERNEL_CASES = [("n", 0, 1, 23, 149), ("n", 0, 2, 23, 150), ("n", 3, 3, 23, 151), ("q", 0, 0, 23, 149)]


@pytest.mark.parametrize("kind,near,effort,h,w", KERNEL_CASES)
def test_kernels_on_caller_made_bytes(gpu_ctx, pkg, oracle, kind, near, effort, h, w):
    """k_index_seed and k_index_chain with the index at base offsets 0 .. 15: what they write, and what they compare, is
    what Python slices out of the index; the guards behind every output stay intact (the entry raises otherwise)."""
    R = 5
    s, ix, _ = _made(gpu_ctx, oracle, kind, near, effort, h, w, R)
    _, ents = _split(ix)
    rec_b, bb = REC_BYTES[kind], _b_bytes(kind, effort, w)
    rng = np.random.default_rng(8)
    avail = 0x1_2345_6789
    residues = set()
    for base in range(16):
        e = 1 + base % len(ents)
        body = np.frombuffer(ents[e - 1], np.uint8)[HEAD:]
        residues.add((base + ix.index(ents[e - 1]) + HEAD) % 16)
        rec, stats, rows = gpu_ctx.debug_index_kernels(ix, base, e, avail=avail)
        want = body[:rec_b].copy()
        want[4:8] = 0                                                    # status kRunning
        want[32:40] = np.frombuffer(struct.pack("<Q", avail), np.uint8)
        want[40:44] = np.frombuffer(struct.pack("<i", 1), np.uint8)
        assert np.array_equal(rec, want), (base, e)
        assert np.array_equal(stats[:bb], body[rec_b:rec_b + bb]) and not stats[bb:].any() and stats.size == 2 * bb, (base, e)
        assert np.array_equal(rows, body[rec_b + bb:rec_b + bb + 2 * w]), (base, e)
        final = (body[:rec_b].copy(), body[rec_b:rec_b + bb].copy() if bb else None, body[rec_b + bb:rec_b + bb + 2 * w].copy())
        final[0][32:64] = rng.integers(0, 256, 32, dtype=np.uint8)       # avail, final_, pad: the host's words, never compared
        assert gpu_ctx.debug_index_kernels(ix, base, e, final=final) == 0, (base, e)
        if kind == "n":
            noisy = final[0].copy()
            noisy[RANK_AT:SYM_AT] = rng.integers(0, 256, SYM_AT - RANK_AT, dtype=np.uint8)
            assert gpu_ctx.debug_index_kernels(ix, base, e, final=(noisy, final[1], final[2])) == 0, ("stale rank bytes", base, e)
        if base % 5 == 2:
            flips = [(0, 0, 1), (0, 8, 1), (0, 16, 1), (0, 28, 1), (0, 64, 1), (0, rec_b - 1, 1), (2, 0, 4), (2, 2 * w - 1, 4), (2, w, 4)]
            flips += [(0, 20, 1 if kind == "n" else 0), (0, 24, 1 if kind == "n" else 0)]          # hi, window: NBLIC only
            if kind == "n":
                flips += [(0, RANK_AT - 1, 1), (0, SYM_AT, 1), (0, RANK_AT, 0), (0, SYM_AT - 1, 0)]
            if bb:
                flips += [(1, 0, 2), (1, bb - 1, 2), (1, bb // 2 + 3, 2)]
            for part, at, code in flips:
                f = [None if p is None else p.copy() for p in final]
                f[part][at] ^= 0x20
                assert gpu_ctx.debug_index_kernels(ix, base, e, final=tuple(f)) == code, (base, e, part, at)
            f = [None if p is None else p.copy() for p in final]
            f[0][100] ^= 1
            f[2][5] ^= 1
            assert gpu_ctx.debug_index_kernels(ix, base, e, final=tuple(f)) == 5
            f = [None if p is None else p.copy() for p in final]
            f[0][4] = 1                                                  # a segment that ended kDone is not a running one
            assert gpu_ctx.debug_index_kernels(ix, base, e, final=tuple(f)) == 1
    assert len(residues) >= 8, residues
    # segment 0: zeros, pos = first_pos, and nothing in B, F or the plane
    rec, stats, rows = gpu_ctx.debug_index_kernels(ix, 3, 0, avail=avail, first_pos=0x77_0000_0010)
    want = np.zeros(rec_b, np.uint8)
    want[8:16] = np.frombuffer(struct.pack("<Q", 0x77_0000_0010), np.uint8)
    want[32:40] = np.frombuffer(struct.pack("<Q", avail), np.uint8)
    want[40] = 1
    assert np.array_equal(rec, want) and not stats.any() and (rows == 0xA7).all()
    # R = 1, entry 1: one row above, at the second half of the slot; the first half of the plane stays as it was
    s1, ix1, _ = _made(gpu_ctx, oracle, kind, near, effort, h, w, 1)
    _, ents1 = _split(ix1)
    body = np.frombuffer(ents1[0], np.uint8)[HEAD:]
    rec, stats, rows = gpu_ctx.debug_index_kernels(ix1, 9, 1, avail=avail)
    assert (rows[:w] == 0xA7).all() and np.array_equal(rows[w:], body[rec_b + bb + w:rec_b + bb + 2 * w])
    final = (body[:rec_b].copy(), body[rec_b:rec_b + bb].copy() if bb else None, body[rec_b + bb + w:rec_b + bb + 2 * w].copy())
    assert gpu_ctx.debug_index_kernels(ix1, 9, 1, final=final) == 0
    final[2][w - 1] ^= 0x80
    assert gpu_ctx.debug_index_kernels(ix1, 9, 1, final=final) == 4


def test_debug_entry_refusals(gpu_ctx, pkg, oracle):
    s, ix, _ = _made(gpu_ctx, oracle, "n", 0, 2, 23, 150, 5)
    _, ents = _split(ix)
    body = np.frombuffer(ents[0], np.uint8)[HEAD:]
    rec_b, bb, w = 86080, 512 * 150, 150
    good = (body[:rec_b].copy(), body[rec_b:rec_b + bb].copy(), body[rec_b + bb:rec_b + bb + 2 * w].copy())
    live = pkg.live_resources()
    broken = bytearray(ix)
    broken[200] ^= 1
    for args, kw in (((bytes(broken), 0, 1), {}), ((ix[:-1], 0, 1), {}), ((ix, 0, 5), {}), ((ix, 0, -1), {}), ((ix, 4097, 1), {}),
                     ((ix, 0, 0), dict(final=good)), ((ix, 0, 1), dict(final=(good[0][:-1], good[1], good[2]))),
                     ((ix, 0, 1), dict(final=(good[0], good[1][:-1], good[2]))), ((ix, 0, 1), dict(final=(good[0], good[1], good[2][:-1]))),
                     ((ix, 0, 1), dict(final=(good[0], None, good[2]))), ((ix, 0, 1), dict(final=(None, good[1], good[2])))):
        with pytest.raises(ValueError):
            gpu_ctx.debug_index_kernels(*args, **kw)
    assert pkg.live_resources() == live
    assert gpu_ctx.debug_index_kernels(ix, 0, 1, final=good) == 0
    assert pkg.live_resources() == live


def test_next_to_encode_batch(gpu_ctx, pkg, oracle):
    a = _made(gpu_ctx, oracle, "n", 1, 2, 120, 300, 16, 12)
    b = _made(gpu_ctx, oracle, "n", 0, 1, 67, 150, 7)
    imgs = [inputs.syn1(64, 96, 40 + k) for k in range(12)]
    want = [oracle.encode(i, 0, 1)[0] for i in imgs]
    got, errs = [], []

    def decode():
        try:
            for _ in range(4):
                got.append(gpu_ctx.decode_batch_indexed([(a[0], a[1]), (b[0], b[1]), (a[0], a[1])]))
        except Exception as e:                                  # pragma: no cover - reported below
            errs.append(e)

    t = threading.Thread(target=decode)
    t.start()
    for _ in range(4):
        assert gpu_ctx.encode_batch(imgs) == want
    t.join()
    assert not errs, errs
    assert len(got) == 4
    for planes in got:
        assert np.array_equal(planes[0], a[2]) and np.array_equal(planes[1], b[2]) and np.array_equal(planes[2], a[2])
