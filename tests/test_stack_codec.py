"""GPU suite (-m gpu): slice stacks through the public calls.  The streams and indexes of ``encode_batch_from(..., stack=...)``
from a [N, D, H, W] uint8 tensor, a D-last (interleaved) view and float16, at efforts 0 .. 3 and through both indexed calls,
are byte for byte those of the same call without ``stack`` on ``stack_forward``'s planes, a sample of them the oracle's;
``decode_batch_into`` / ``decode_batch_indexed_into`` with the modes return the original slices into uint8 [N, D, H, W], a
D-last tensor and float16 with a scale and bias per slice, whole, as a row range, as a column window, and one slice through
its run with the others skipped; ``stack_plan`` on the four constructed classes; a stream cut short in the middle of a run;
and what is refused."""
import numpy as np
import pytest

import stack_inputs as si
from test_decode_to_device import _bits, _elements, _filled
from test_deliver_strided_host import PATTERN
from test_rct_codec import _dev, _torch

pytestmark = pytest.mark.gpu

GEOMS = ((48, 80), (33, 17))
DEPTH = 5
N = 2                                                          # stacks per call
EVERY = 16
PAT = {name: si.modes_of(name, DEPTH) for name in si.PATTERNS}  # stack_inputs' four patterns at this depth
MIXED = [0, 1, 1, 0, 1, 0, 0, 1, 1, 1]                          # runs [0 1 2] [3 4] in stack 0, a lone key slice and the run [1 2 3 4] in stack 1
LAST = PAT["a key in the middle"] + PAT["a key last"]           # runs [0 1] [2 3 4] in stack 0, the run [0 1 2 3] and a lone key slice BEHIND it in stack 1
MODES = ("delta", MIXED, PAT["all keys"] * N, LAST)
assert PAT["all deltas"] == [0, 1, 1, 1, 1] and LAST == [0, 1, 0, 1, 1, 0, 1, 1, 1, 0]


def _runs(modes):
    """[(first image, length)] of the runs of a call's mode bytes."""
    return [(s * DEPTH + d, n) for s in range(len(modes) // DEPTH) for d, n in si.runs_of(modes[s * DEPTH:(s + 1) * DEPTH])]


_cache = {}


@pytest.fixture(scope="module")
def ctx(pkg, gpu_ctx):
    """A context of this module's own (made after the session's, which initialises torch first)."""
    c = pkg.Context(device=0, n_slots=3, n_coders=3)
    yield c
    c.close()


def _volumes(h, w):
    """[N, DEPTH, h, w] uint8: stack 0 of the static class, stack 1 of the cut class."""
    if (h, w) not in _cache:
        stacks = si.class_stacks(h, w, depth=DEPTH, seed=70)
        _cache[(h, w)] = np.ascontiguousarray(stacks[[0, 2]])
    return _cache[(h, w)]


def _bytes_of(stack, n=N * DEPTH):
    return [0 if k % DEPTH == 0 else 1 for k in range(n)] if isinstance(stack, str) else list(stack)


def _planes(pkg, vol, modes):
    """The N * DEPTH planes whose streams stack=modes writes, n-major."""
    return [p for s in range(len(vol)) for p in pkg.stack_forward(list(vol[s]), modes[s * DEPTH:(s + 1) * DEPTH])]


def _source(vol, layout):
    """(what encode_batch_from takes, scale): the volumes in device memory in one of three layouts."""
    if layout == "ndhw uint8":
        return _dev(vol), 1.0
    if layout == "d-last uint8":
        return _dev(vol.transpose(0, 2, 3, 1)).permute(0, 3, 1, 2), 1.0
    return _dev((vol.astype(np.float32) / 255.0).astype(np.float16)), 255.0      # (|f16(p / 255) * 255 - p| < 255 * 2^-11: the collected plane is the slice)


def _pairs(ctx, pkg, streams, Rs=(7, 5, 16)):
    """(stream, index) per plane: another R for neighbouring slices, packed and unpacked indexes mixed."""
    out = []
    for k, s in enumerate(streams):
        ix = ctx.build_index(s, Rs[k % 3])
        out.append((s, pkg.pack_index(ix) if k % 2 else ix))
    return out


def _decode(ctx, how, pairs, out, stack, **kw):
    if how == "indexed":
        return ctx.decode_batch_indexed_into(pairs, out, stack=stack, **kw)
    return ctx.decode_batch_into([s for s, _ in pairs], out, stack=stack, **kw)


@pytest.mark.parametrize("effort", (0, 1, 2, 3))
@pytest.mark.parametrize("geom", GEOMS)
def test_streams_and_indexes_are_those_of_the_forward_planes(ctx, pkg, oracle, geom, effort):
    h, w = geom
    vol = _volumes(h, w)
    assert _bytes_of("delta") == PAT["all deltas"] * N
    for stack in ("delta", MIXED, LAST) if effort < 2 else ("delta", LAST):
        modes = _bytes_of(stack)
        planes = _planes(pkg, vol, modes)
        dev_planes = _dev(np.stack(planes))
        want = ctx.encode_batch_from(dev_planes, effort=effort)
        assert all(s is not None for s in want) and len(want) == N * DEPTH
        for layout in ("ndhw uint8", "d-last uint8", "float16"):
            src, scale = _source(vol, layout)
            assert ctx.encode_batch_from(src, scale=scale, effort=effort, stack=stack) == want, (layout, stack)
        src, _ = _source(vol, "d-last uint8")
        assert ctx.encode_batch_from([src[n][d] for n in range(N) for d in range(DEPTH)], effort=effort, stack=np.array(modes, np.uint8), depth=DEPTH) == want
        if effort < 2:                                         # both indexed calls
            want_x = ctx.encode_batch_from(dev_planes, effort=effort, every_rows=EVERY, band_rows=5)
            assert all(s is not None and x is not None for s, x in want_x)
            for layout in ("ndhw uint8", "float16"):
                src, scale = _source(vol, layout)
                assert ctx.encode_batch_from(src, scale=scale, effort=effort, every_rows=EVERY, band_rows=5, stack=stack) == want_x, (layout, stack)
        for k in (0, 1, DEPTH + 3, N * DEPTH - 1):             # a key slice, two delta slices and the call's last slice against the oracle
            assert want[k] == (oracle.qencode(planes[k]) if effort == 0 else oracle.encode(planes[k], 0, effort)[0]), k
        assert ctx.encode_batch_from(_dev(vol), effort=effort)[1] != want[1]      # the difference took place
    if effort == 1:                                            # a stack of keys only is DEPTH images like any other
        assert ctx.encode_batch_from(_dev(vol), stack=MODES[2]) == ctx.encode_batch_from(_dev(vol))


@pytest.mark.parametrize("how", ("plain", "indexed"))
@pytest.mark.parametrize("geom", GEOMS)
def test_decode_gives_the_original_slices(ctx, pkg, geom, how):
    h, w = geom
    vol = _volumes(h, w)
    scales = [1.0 / 255.0 * (1 + k % 3) for k in range(N * DEPTH)]
    biases = [-0.5 + 0.25 * (k % 4) for k in range(N * DEPTH)]
    for stack in MODES:
        modes = _bytes_of(stack)
        # (without an index the slices of a run may be of different efforts: their planes lie in chunks of both streams)
        streams = ctx.encode_batch_from(_dev(vol), stack=stack, effort=1 if stack == "delta" or how == "indexed" else [1 + k % 2 for k in range(N * DEPTH)])
        assert all(s is not None for s in streams)
        pairs = _pairs(ctx, pkg, streams)
        out = _filled((N, DEPTH, h, w), 0)
        info = {}
        assert _decode(ctx, how, pairs, out, stack, info=info) == [0] * (N * DEPTH) and info["rc"] == 0
        assert np.array_equal(_bits(out), vol), (how, stack)
        last = _filled((N, h, w, DEPTH), 0)                    # D-last: the slices interleaved pixel by pixel
        assert _decode(ctx, how, pairs, last.permute(0, 3, 1, 2), np.array(modes, np.uint8)) == [0] * (N * DEPTH)
        assert np.array_equal(_bits(last), vol.transpose(0, 2, 3, 1)), (how, stack)
        half = _filled((N, DEPTH, h, w), 1)
        assert _decode(ctx, how, pairs, half, stack, scale=scales, bias=biases) == [0] * (N * DEPTH)
        got = _bits(half)
        for k in range(N * DEPTH):
            assert np.array_equal(got[k // DEPTH, k % DEPTH], _elements(vol[k // DEPTH, k % DEPTH], 1, scales[k], biases[k])), (how, stack, k)
        # a row range (with an index it chooses the segments, another R in every slice) and a column window
        r, c_ = (12, h - 1), (5, w - 3)
        win = _filled((N, DEPTH, r[1] - r[0], c_[1] - c_[0]), 1)
        assert _decode(ctx, how, pairs, win, stack, rows=r, cols=c_, scale=scales, bias=biases) == [0] * (N * DEPTH)
        got = _bits(win)
        for k in range(N * DEPTH):
            assert np.array_equal(got[k // DEPTH, k % DEPTH], _elements(vol[k // DEPTH, k % DEPTH, r[0]:r[1], c_[0]:c_[1]], 1, scales[k], biases[k])), (how, stack, k)


@pytest.mark.parametrize("modes", (MIXED, LAST), ids=("mixed", "key-last"))
@pytest.mark.parametrize("how", ("plain", "indexed"))
def test_one_slice_through_its_run(ctx, pkg, how, modes):
    """Random access: the streams key .. target of one run with one destination, the others None; and a whole call with
    skipped slices among delivered ones."""
    h, w = GEOMS[0]
    vol = _volumes(h, w)
    streams = ctx.encode_batch_from(_dev(vol), stack=modes)
    pairs = _pairs(ctx, pkg, streams)
    runs = _runs(modes)
    # the last slice of every run (a lone key slice is a run of one), and the second slice of the longest one
    first, n = max(runs, key=lambda r: r[1])
    for first, target in [(f, f + n - 1) for f, n in runs] + [(first, first + 1)]:
        run = pairs[first:target + 1]
        n = len(run)
        out = _filled((h, w), 0)
        run_modes = [0] + [1] * (n - 1)
        info = {}
        assert _decode(ctx, how, run, [None] * (n - 1) + [out], run_modes, depth=n, info=info) == [0] * n and info["rc"] == 0
        assert np.array_equal(_bits(out), vol[target // DEPTH, target % DEPTH]), (how, first, target)
    outs = [None if k % 3 == 1 else _filled((h, w), 0) for k in range(N * DEPTH)]
    assert _decode(ctx, how, pairs, outs, modes, depth=DEPTH) == [0] * (N * DEPTH)
    for k, o in enumerate(outs):
        assert o is None or np.array_equal(_bits(o), vol[k // DEPTH, k % DEPTH]), (how, k)
    before = ctx.stack_plan_stats()
    assert _decode(ctx, how, pairs, _filled((N, DEPTH, h, w), 0), modes) == [0] * (N * DEPTH)
    after = ctx.stack_plan_stats()
    assert after["deliver_launches"] == before["deliver_launches"] + 1 and after["runs"] == before["runs"] + sum(n > 1 for _, n in runs) == before["runs"] + 3
    assert ctx.deliver_stats()[0] == sum(n == 1 for _, n in runs) == 1      # and the lone key slice through k_deliver


def test_the_plan_on_the_classes(ctx, pkg):
    h, w, depth = 96, 80, 6
    stacks = si.class_stacks(h, w, depth)
    want = [m for modes in si.class_modes(depth) for m in modes]
    numpy_costs = np.concatenate([pkg.stack_cost_numpy(list(s)) for s in stacks])
    for layout in ("ndhw uint8", "d-last uint8", "float16"):
        src, scale = _source(stacks, layout)
        before = ctx.stack_plan_stats()
        modes, costs = ctx.stack_plan(src, scale=scale, costs=True)
        after = ctx.stack_plan_stats()
        assert modes.tolist() == want, layout
        assert np.array_equal(costs, numpy_costs), layout
        assert after["cost_launches"] == before["cost_launches"] + 1 and after["elements"] == before["elements"] + stacks.size and after["plan_ms"] > 0
    assert ctx.stack_plan(_dev(stacks), key_every=2).tolist() == [m if d % 2 else 0 for m, d in zip(want, list(range(depth)) * 4)]
    assert ctx.stack_plan([t for s in _dev(stacks) for t in s], depth=depth).tolist() == want
    # the planned streams are those of the forward planes, and come back
    streams = ctx.encode_batch_from(_dev(stacks), stack=modes)
    planes = [p for s in range(4) for p in pkg.stack_forward(list(stacks[s]), want[s * depth:(s + 1) * depth])]
    assert streams == ctx.encode_batch_from(_dev(np.stack(planes)))
    out = _filled(stacks.shape, 0)
    assert ctx.decode_batch_into(streams, out, stack=modes) == [0] * (4 * depth)
    assert np.array_equal(_bits(out), stacks)
    size = lambda stack: sum(len(s) for s in ctx.encode_batch_from(_dev(stacks), stack=stack))
    print("stream bytes: keys %d, delta %d, planned %d" % (size(None), size("delta"), size(modes)))
    # a stack with a refused source, and one of unequal sizes: 0xFF for its slices alone
    views = [t for s in _dev(stacks) for t in s]
    views[depth + 2] = views[depth + 2][:, :w - 1]
    modes, costs = ctx.stack_plan(views, depth=depth, costs=True)
    assert modes.tolist() == want[:depth] + [pkg.STACK_REFUSED] * depth + want[2 * depth:] and not costs[depth:2 * depth].any()
    assert np.array_equal(costs[:depth], numpy_costs[:depth])
    for bad in (dict(depth=5), dict(depth=0), dict(depth=depth, key_every=-1), dict(depth=depth, scale=float("nan"))):
        with pytest.raises(ValueError):
            ctx.stack_plan([t for s in _dev(stacks) for t in s], **bad)


@pytest.mark.parametrize("modes", (MIXED, LAST), ids=("mixed", "key-last"))
@pytest.mark.parametrize("how", ("plain", "indexed"))
def test_a_stream_cut_short_in_the_middle_of_a_run(ctx, pkg, how, modes):
    """Earlier slices are right, that slice and the later ones of its run are zeros with -1, the next run -- a lone key slice
    behind the run among them -- and the other stack are right."""
    from test_indexed_batch_decode import _forge
    h, w = GEOMS[0]
    vol = _volumes(h, w)
    streams = ctx.encode_batch_from(_dev(vol), stack=modes)
    pairs = _pairs(ctx, pkg, streams, Rs=(7, 7, 7))

    def damaged(k):
        out = list(pairs)
        if how == "plain":
            out[k] = (streams[k][:len(streams[k]) * 2 // 3], pairs[k][1])
            assert ctx.decode_batch([out[k][0]])[0] is None
        else:
            forged = _forge(ctx.build_index(streams[k], 7), 4, "n", 1, w, "row1")
            assert pkg.check_index(forged, streams[k])
            out[k] = (streams[k], forged)
        return out

    runs = _runs(modes)
    cases = [(f + n // 2, tuple(range(f + n // 2, f + n))) for f, n in runs] + [(runs[0][0], tuple(range(runs[0][0], runs[0][0] + runs[0][1])))]      # the middle of every run; a key
    if modes is MIXED:
        assert (1, (1, 2)) in cases and (DEPTH + 3, (DEPTH + 3, DEPTH + 4)) in cases and (DEPTH, (DEPTH,)) in cases
    else:
        assert (DEPTH + 2, (DEPTH + 2, DEPTH + 3)) in cases and (N * DEPTH - 1, (N * DEPTH - 1,)) in cases      # the run in front of the last key stops there
    for k, bad in cases:
        out = _filled((N, DEPTH, h, w), 0)
        info = {}
        want = [-1 if i in bad else 0 for i in range(N * DEPTH)]
        assert _decode(ctx, how, damaged(k), out, modes, info=info) == want and info["rc"] == -1, (how, k)
        got = _bits(out)
        for i in range(N * DEPTH):
            assert np.array_equal(got[i // DEPTH, i % DEPTH], vol[i // DEPTH, i % DEPTH] if want[i] == 0 else np.zeros((h, w), np.uint8)), (how, k, i)
    # a damaged slice that is skipped has its plane's status, and the delivered slices behind it have none of its pixels
    k, bad = cases[0]                                           # slice 1: the middle of the run [0 1 2], or the end of the run [0 1]
    outs = [None if i == k else _filled((h, w), 0) for i in range(N * DEPTH)]
    assert _decode(ctx, how, damaged(k), outs, modes, depth=DEPTH) == [-1 if i in bad else 0 for i in range(N * DEPTH)]
    for i, o in enumerate(outs):
        assert o is None or np.array_equal(_bits(o), np.zeros((h, w), np.uint8) if i in bad else vol[i // DEPTH, i % DEPTH]), (how, i)


def test_refusals(ctx, pkg):
    h, w = GEOMS[0]
    vol = _volumes(h, w)
    src = _dev(vol)
    good = MODES[1]
    streams = ctx.encode_batch_from(src, stack=good)
    pairs = _pairs(ctx, pkg, streams)
    # call level: an invalid byte, a delta at the head of a stack, a depth that does not divide -- nothing is written
    for bad in ([0, 2] + [0] * 8, [0] * 5 + [1] + [0] * 4, [0, 0xFF] + [0] * 8):
        for kw in ({}, dict(effort=0), dict(every_rows=EVERY), dict(effort=0, every_rows=EVERY)):
            with pytest.raises(ValueError):
                ctx.encode_batch_from(src, stack=bad, **kw)
        for how in ("plain", "indexed"):
            out = _filled((N, DEPTH, h, w), 0)
            info = {}
            assert _decode(ctx, how, pairs, out, bad, info=info) == [-1] * (N * DEPTH) and info["rc"] == -1
            assert (_bits(out) == PATTERN).all()
    views = [src[n][d] for n in range(N) for d in range(DEPTH)]
    for bad in (dict(stack=good, depth=3), dict(stack=good, depth=0), dict(stack=good), dict(stack=[0] * 9, depth=DEPTH), dict(stack="keys", depth=DEPTH),
                dict(stack=good, depth=DEPTH, color="rct"), dict(depth=DEPTH)):
        with pytest.raises(ValueError):
            ctx.encode_batch_from(views, **bad)
    with pytest.raises(ValueError):
        ctx.encode_batch_from(src, stack=good, recon_out=_filled((N, DEPTH, h, w), 0))
    with pytest.raises(ValueError):
        ctx.decode_batch_into(streams, _filled((N, DEPTH, h, w), 0), stack=good, color="rct")
    # the C calls themselves: the flag in a _stack call, a count the depth does not divide
    srcs, fmt = pkg._srcs_of(views, None, None)
    for kw in ({}, dict(effort=0), dict(every_rows=EVERY), dict(effort=0, every_rows=EVERY)):
        with pytest.raises(ValueError):
            ctx.encode_from_srcs(srcs, fmt | pkg.FORMAT_RCT, stack=(DEPTH, good), **kw)
        with pytest.raises(ValueError):
            ctx.encode_from_srcs(srcs[:9], fmt, stack=(DEPTH, good[:9]), **kw)
        with pytest.raises(ValueError):
            ctx.encode_from_srcs(srcs, fmt, stack=(0, good), **kw)
    assert ctx.encode_from_srcs(srcs, fmt, stack=(DEPTH, good)) == streams
    # near > 0: on a key slice whose successor is a key slice (stack 1, slice 0) it is an image like any other; anywhere else it refuses the call
    near = [0] * (N * DEPTH)
    near[DEPTH] = 2
    got = ctx.encode_batch_from(src, near=near, stack=good)
    assert all(s is not None for s in got) and got[:DEPTH] == streams[:DEPTH] and got[DEPTH + 1:] == streams[DEPTH + 1:] and got[DEPTH] != streams[DEPTH]
    out = _filled((N, DEPTH, h, w), 0)
    assert ctx.decode_batch_into(got, out, stack=good) == [0] * (N * DEPTH)
    assert np.array_equal(_bits(out)[0], vol[0]) and np.abs(_bits(out)[1, 0].astype(int) - vol[1, 0]).max() <= 2
    for k in (1, 0, 3, DEPTH + 2, DEPTH + 1):                  # a delta slice, or a key slice with a delta slice behind it
        bad_near = [0] * (N * DEPTH)
        bad_near[k] = 1
        with pytest.raises(ValueError):
            ctx.encode_batch_from(src, near=bad_near, stack=good)
        with pytest.raises(ValueError):
            ctx.encode_from_srcs(srcs, fmt, near=bad_near, stack=(DEPTH, good))
    # a near-lossless stream inside a run refuses its stack on decode; the other stack is delivered
    lossy = ctx.encode_batch_from(_dev(np.stack(_planes(pkg, vol, _bytes_of(good)))), near=[0, 0, 1] + [0] * 7)
    out = _filled((N, DEPTH, h, w), 0)
    assert ctx.decode_batch_into(lossy, out, stack=good) == [-1] * DEPTH + [0] * DEPTH
    assert (_bits(out)[0] == PATTERN).all() and np.array_equal(_bits(out)[1], vol[1])
    # stack level: a member that does not parse, unequal sizes, unequal windows, a refused destination -- that stack alone, nothing written
    other = ctx.encode_batch_from(_dev(vol[:1, :1, :h - 1]))[0]
    for how in ("plain", "indexed"):
        for case in ("garbage", "size", "window", "dest"):
            p = list(pairs)
            outs = [_filled((h, w), 0) for _ in range(N * DEPTH)]
            rows = None
            if case == "garbage":
                p[2] = (b"not a stream", pairs[2][1])
            elif case == "size":
                p[2] = (other, ctx.build_index(other, 7))
                outs[2] = _filled((h - 1, w), 0)
            elif case == "window":
                rows = [(0, 0)] * (N * DEPTH)
                rows[2] = (1, h)
                outs[2] = _filled((h - 1, w), 0)
            else:
                outs[2] = _filled((h, w - 1), 0)                # not its window's shape: refused
            info = {}
            assert _decode(ctx, how, p, outs, good, depth=DEPTH, rows=rows, info=info) == [-1] * DEPTH + [0] * DEPTH and info["rc"] == -1, (how, case)
            assert all((_bits(o) == PATTERN).all() for o in outs[:DEPTH]), (how, case)
            assert all(np.array_equal(_bits(o), vol[1, d]) for d, o in enumerate(outs[DEPTH:])), (how, case)
    # the encoder: a stack with a delta and a source of another size is refused as a whole, the other stack is coded
    views[2] = views[2][:, :w - 1]
    got = ctx.encode_batch_from(views, stack=good, depth=DEPTH)
    assert got[:DEPTH] == [None] * DEPTH and got[DEPTH:] == streams[DEPTH:]
