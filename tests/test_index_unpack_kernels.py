"""GPU suite (-m gpu): k_index_unpack_scan, k_index_unpack and k_index_unpack_rank on packings the library's writer never
makes (index_pack_inputs.py; test_index_pack_inputs_host.py says which paths they reach): every width byte 0 .. 8 unit of
every unit, fields of 33 .. 64 bits at every shift, raw parts in front of coded ones, the rank bytes raw, a raw body in the
middle of a chain, symbol bytes with repeats and values of 20 and more, full-range unit-2 differences.  The kernels run
alone through nblic_amd_debug_index_unpack, which accepts what the structural walk accepts, and the bodies they store are
compared byte for byte with the bodies the indexes were BUILT FROM: no reader is involved, and there is no tolerance.  Then
the same kinds of packing of real indexes go through the public calls."""
import ctypes as C
import struct

import numpy as np
import pytest

import index_pack_inputs as ipi
from test_index_pack import MODES, SIZES, _live
from test_index_pack_host import rehash_entries
from test_seek_index import _stream

pytestmark = pytest.mark.gpu

CASES = ipi.case_ids()
case_id = lambda c: "%dx%d-%d-k%de%d-%s-%s" % (c[0] + c[1] + c[2:])
PATTERN = 0xA7


def tab_of(case):
    """RecordLayout::tab: the bytes of a body the device holds (all of it but the QNBLIC tables)."""
    (_, w, _), (kind, effort) = case[0], case[1]
    return 12352 + 2 * w if kind else 86080 + {1: 0, 2: 512, 3: 1024}[effort] * w + 2 * w


def truth_of(case):
    c = ipi.cases()[case]
    if "truth" not in c:
        c["truth"] = np.frombuffer(b"".join(c["bodies"]), np.uint8).reshape(len(c["bodies"]), -1)[:, :tab_of(case)]
    return c["truth"]


def check_task(case, result, walk, first_out, what):
    bodies, guard = result
    tab, truth = tab_of(case), truth_of(case)
    assert bodies.shape == (walk - first_out, (tab + 15) & ~15), what
    assert (guard == PATTERN).all(), what                                      # every byte behind out_stride x entries
    for e in range(first_out, walk):                                           # [tab, out_stride) is not compared
        got = bodies[e - first_out, :tab]
        if not np.array_equal(got, truth[e]):
            at = np.flatnonzero(got != truth[e])
            raise AssertionError("%s: entry %d differs at %d bytes, first at %d (%#x, built from %#x)" % (what, e, at.size, at[0], got[at[0]], truth[e][at[0]]))


def pairs_of(count):
    return [(count, 0), (count, count - 1), (1, 0), (4, 2)]


# ---- a. the hook against construction ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_unpacked_bodies_are_the_bodies_the_index_was_built_from(gpu_ctx, pkg, case):
    c = ipi.cases()[case]
    count = len(c["bodies"])
    with _live(pkg):
        for base in ipi.BASE_OFFSETS:
            for walk, first_out in pairs_of(count):
                (result,) = gpu_ctx.debug_index_unpack([(c["packed"], base, walk, first_out)])
                check_task(case, result, walk, first_out, (case, base, walk, first_out))


# ---- b. several tasks in one launch ------------------------------------------------------------------------------------------
def test_five_tasks_with_rank_group_ties(gpu_ctx, pkg):
    """QNBLIC tasks have no rank groups: first_rank_group ties at the front, in the middle and at the end of the launch."""
    order = [(((37, 29, 5), (1, 0), "graded", "mix"), 1, 7, 0), (((13, 161, 1), (0, 1), "graded", "mix"), 2, 12, 5),
             (((13, 161, 1), (1, 0), "graded", "min"), 3, 1, 0), (((37, 30, 5), (0, 3), "graded", "mix"), 0, 4, 2),
             (((37, 30, 5), (1, 0), "real", "rand"), 1, 7, 6)]
    assert [k[1][0] for k, _, _, _ in order] == [1, 0, 1, 0, 1]
    with _live(pkg):
        results = gpu_ctx.debug_index_unpack([(ipi.cases()[k]["packed"], base, walk, first) for k, base, walk, first in order])
        again = gpu_ctx.debug_index_unpack([(ipi.cases()[k]["packed"], base, walk, first) for k, base, walk, first in reversed(order)])
    for (k, base, walk, first), r in zip(order, results):
        check_task(k, r, walk, first, (k, base, walk, first))
    for (k, base, walk, first), r in zip(reversed(order), again):
        check_task(k, r, walk, first, ("reversed", k, base, walk, first))
    with _live(pkg):                                                           # eight tasks, the most a call takes
        eight = [order[i % 5] for i in range(8)]
        for (k, base, walk, first), r in zip(eight, gpu_ctx.debug_index_unpack([(ipi.cases()[k]["packed"], base, walk, first) for k, base, walk, first in eight])):
            check_task(k, r, walk, first, ("eight", k))


# ---- d. agreement with the host ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo_mode", ipi.GEOMETRIES, ids=lambda g: "%dx%d-%d-k%de%d" % (g[0] + g[1]))
def test_the_hook_and_the_host_reader_agree(gpu_ctx, pkg, geo_mode):
    for case in CASES:
        if case[:2] != geo_mode:
            continue
        packed = ipi.cases()[case]["packed"]
        ix = pkg.unpack_index(packed)
        count = struct.unpack_from("<i", ix, 40)[0]
        eb = (len(ix) - 96 - 32) // count
        (bodies, guard), = gpu_ctx.debug_index_unpack([(packed, 3, count, 0)])
        tab = tab_of(case)
        for e in range(count):
            host = ix[96 + e * eb + 8 + 168:96 + e * eb + 8 + 168 + tab]
            assert bodies[e, :tab].tobytes() == host, (case, e)


# ---- e. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(gpu_ctx, pkg):
    case = ((37, 29, 5), (0, 2), "graded", "min")
    packed = ipi.cases()[case]["packed"]
    lib, count = pkg.load_library(), 7
    entries = ipi.walk(packed)
    code, unit, flag, at, widths = entries[1][1][1]                            # the contexts of entry 1: a width byte of 33, every hash made right
    assert (code, unit, flag) == ("diff", 4, 1) and widths[0] <= 32
    flipped = bytearray(packed)
    flipped[at] = 33
    flipped = rehash_entries(bytes(flipped))
    too_long = bytearray(packed)
    too_long[at + 5] ^= 1                                                      # another width byte: the payloads no longer end at the seal
    too_long = rehash_entries(bytes(too_long))
    bad_head = bytearray(packed)
    struct.pack_into("<i", bad_head, 44, 1)                                    # a reserved field of the head: the walk does not look, the head check does
    bad_head = rehash_entries(bytes(bad_head))
    assert pkg.load_library().nblic_amd_index_unpacked_bytes(np.frombuffer(bad_head, np.uint8).ctypes.data, len(bad_head)) > 0
    refused = [[(packed, 0, 0, 0)], [(packed, 0, count + 1, 0)], [(packed, 0, count, count)], [(packed, 0, 3, 3)], [(packed, 0, 3, -1)],
               [(packed, 4097, count, 0)], [(flipped, 0, count, 0)], [(too_long, 0, count, 0)], [(bad_head, 0, count, 0)], [(packed[:-1], 0, count, 0)],
               [(ipi.cases()[case]["index"], 0, count, 0)], [(packed, 0, count, 0), (flipped, 0, 1, 0)], [], [(packed, 0, 1, 0)] * 9]
    for tasks in refused:
        before = pkg.live_resources()
        with pytest.raises(ValueError):
            gpu_ctx.debug_index_unpack(tasks)
        assert pkg.live_resources() == before
    before = pkg.live_resources()
    x = np.frombuffer(packed, np.uint8)
    out = np.zeros(16, np.uint8)                                               # a cap too small, a null pointer, no context: the return code itself
    one = lambda v, t: (t * 1)(v)
    args = lambda cap, outp: (one(x.ctypes.data, C.c_void_p), one(x.size, C.c_size_t), one(0, C.c_size_t), one(1, C.c_int), one(0, C.c_int),
                              one(outp, C.c_void_p), one(cap, C.c_size_t), one(0, C.c_size_t))
    assert lib.nblic_amd_debug_index_unpack(gpu_ctx.handle, 1, *args(16, out.ctypes.data)) == -1
    assert lib.nblic_amd_debug_index_unpack(gpu_ctx.handle, 1, *args(1 << 20, None)) == -1
    assert lib.nblic_amd_debug_index_unpack(None, 1, *args(16, out.ctypes.data)) == -1
    assert lib.nblic_amd_debug_index_unpack(gpu_ctx.handle, 1, None, None, None, None, None, None, None, None) == -1
    assert pkg.live_resources() == before
    (result,) = gpu_ctx.debug_index_unpack([(packed, 0, count, 0)])            # and the context still works
    check_task(case, result, count, 0, "after the refusals")


# ---- c. the public calls on non-canonical packings of real indexes -----------------------------------------------------------
_real = {}


def _made(gpu_ctx, oracle):
    """{(mode, size): (stream, index, reconstruction)} as test_index_pack.py makes them, the first two sizes."""
    if not _real:
        keys = [(m, g) for m in MODES for g in SIZES[:2]]
        streams = [_stream(oracle, *m, g[0], g[1]) for m, g in keys]
        indexes = gpu_ctx.build_index_batch([s for s, _ in streams], [g[2] for _, g in keys])
        for key, (s, rec), ix in zip(keys, streams, indexes):
            assert ix is not None, key
            _real[key] = (s, ix, rec)
    return _real


def _ranges(h, R):
    last, mid = ((h - 1) // R) * R, ((h - 1) // R // 2) * R
    return [(0, 1), (1, min(h, 2 * R + 1)), (mid - 1, min(h, mid + R + 1)), (last, h), (last - 1, h), (0, h)]


@pytest.mark.parametrize("packing", ["full", "rand", "mix"])
def test_public_calls_take_non_canonical_packings(gpu_ctx, pkg, oracle, packing):
    made = _made(gpu_ctx, oracle)
    keys = list(made)
    packed = {}
    for k, key in enumerate(keys):
        s, ix, _ = made[key]
        p = ipi.pack(ix, ipi.chooser(packing, ix), np.random.default_rng(900 + k))
        assert p != pkg.pack_index(ix) and pkg.check_index(p, s) and pkg.unpack_index(p) == ix, key
        packed[key] = p
    if packing == "mix":                                                       # the rank bytes raw, a raw body neither first nor last
        for key in keys:
            entries = ipi.walk(packed[key])
            assert [e for e, (flag, _) in enumerate(entries) if flag == 0] == [len(entries) // 2], key
            assert key[0][0] == "q" or any(flag == 0 for body, row in entries if body for code, _, flag, _, _ in row if code == "rank"), key
    pairs, rows, want = [], [], []
    for key in keys:
        s, ix, rec = made[key]
        for r in _ranges(key[1][0], key[1][2]):
            pairs.append((s, packed[key])); rows.append(r); want.append(rec[r[0]:r[1]])              # the oracle's rows
            assert np.array_equal(gpu_ctx.decode_rows(s, ix, *r), want[-1]), (key, r)
    mixed = []
    for k, key in enumerate(keys):                                             # non-canonical, canonical and unpacked in one call
        s, ix, _ = made[key]
        mixed.append((s, (packed[key], pkg.pack_index(ix), ix)[k % 3]))
    for segments in (3, 0):                                                    # rounds that start above segment 0; one round
        gpu_ctx.set_index_round(segments)
        try:
            with _live(pkg):
                info = {}
                planes = gpu_ctx.decode_batch_indexed([(made[key][0], packed[key]) for key in keys], info=info)
                got = gpu_ctx.decode_batch_indexed(pairs, rows)
                both = gpu_ctx.decode_batch_indexed(mixed)
        finally:
            gpu_ctx.set_index_round(0)
        assert info["rc"] == 0 and info["status"] == [0] * len(keys), segments
        for key, plane, other in zip(keys, planes, both):
            assert plane is not None and np.array_equal(plane, made[key][2]), (key, segments)
            assert other is not None and np.array_equal(other, made[key][2]), (key, segments, "mixed")
        for g, wnt, r in zip(got, want, rows):
            assert g is not None and np.array_equal(g, wnt), (r, segments)
    for mode in MODES:
        s, ix, rec = made[(mode, SIZES[0])]
        with _live(pkg):
            assert np.array_equal(gpu_ctx.decode_indexed(s, packed[(mode, SIZES[0])]), rec), mode
            assert np.array_equal(gpu_ctx.decode_rows(s, packed[(mode, SIZES[0])], 11, 23), rec[11:23]), mode
