"""GPU suite (-m gpu): no result depends on what earlier calls left in a context's workspaces.

Every device buffer of a context is grow-only and reused from call to call, and the kernels are written on the premise that
stale bytes may be read but never used ("Device allocations": which buffer is scratch, which is carried state,
and who initialises or gates it).  The rest of the suite runs its cases in whatever state its shared context happens to be in,
nearly always a smaller image before a larger one; here every SUBJECT of tests/history_inputs.py -- small encodes and decodes
in every mode, the stage arrays, the kernels on caller-made records, bands, index, plans, collection and delivery -- runs behind
every PREDECESSOR: ordinary calls that leave large, hostile, flat, effort-0, serial, decoded and planned work behind, or a dead context's
(tests/test_workspace_history_host.py proves on the CPU that they are what they claim).  Each subject runs twice in a row and
is held to an expectation computed once on the CPU: the oracle's streams and arrays, the host walks, the checkers of the
kernels' own test files.  Every assertion is equality.

``Context.debug_workspaces()`` proves that a subject really ran in the predecessor's memory: capacities and addresses behind
every subject equal those behind the predecessor, or the case fails -- a buffer that was reallocated proves nothing.  To
make that deterministic the contexts have five coder threads: with at most ten images outstanding no launch of these tests is
packed (pipeline.hip launch_back), so every image takes a coded-bin buffer of the pool, whose front the predecessor's first
launch has allocated; packs have a test of their own."""
import functools

import numpy as np
import pytest

import chain_inputs as ci
import entropy_inputs as ei
import history_inputs as hi
import inputs

pytestmark = pytest.mark.gpu

N_CODERS = 5                                                   # 2 x 5 = 10 >= the images of any call of these contexts: no packs
SLOT_KEYS = ("px_cap", "ev_cap", "pool_bytes", "rec1", "events")
SLOT_LAZY = ("img",)                                           # allocated by the first call that needs one: compared once it exists
# (recon and stats are reported and not compared: they are sized by the width and the effort of the serial-mode image a slot
# coded last, a launch holds the images of ONE effort, and so the four images of `serial` reach slots 0 and 1 alone)
CTX_KEYS = ("cbufs", "cbufs_held", "cbufs_cap", "pbufs", "pbufs_held", "pbufs_cap")
CTX_LAZY = ("dec_arena", "dec_jobs")


@pytest.fixture(scope="module")
def live(gpu_ctx, pkg):
    """What the library holds before this module's first context is what it holds after the last one is closed.  (gpu_ctx
    first: torch initialises HIP before the library does.  Its coder threads create their events after the context exists,
    so when this module is the session's first the shared context works once, and one context comes and goes, before the
    count is taken.)"""
    for _ in range(4):
        gpu_ctx.debug_stage(inputs.make("noise", 17, 13), "coded")
    gpu_ctx.encode_batch([i for _, i in hi.subject_images()])
    make_ctx(pkg).close()
    before = pkg.live_resources()
    yield before
    assert pkg.live_resources() == before


def make_ctx(pkg, n_groups=1, **kw):
    return pkg.Context(device=0, n_slots=8, n_coders=kw.pop("n_coders", N_CODERS), n_groups=n_groups, **kw)


def moved(before, after, arenas=False):
    """What was reallocated between two reports of ``debug_workspaces`` (empty: nothing).  ``arenas``: the decode arenas too
    -- behind the ``decode`` predecessor, which is the one that leaves arenas larger than the subjects need."""
    out = []
    for g, (gb, ga) in enumerate(zip(before["slots"], after["slots"])):
        for k, (b, a) in enumerate(zip(gb, ga)):
            out += [(g, k, key, b[key], a[key]) for key in SLOT_KEYS if b[key] != a[key]]
            out += [(g, k, key, b[key], a[key]) for key in SLOT_LAZY if b[key] and b[key] != a[key]]
    b, a = before["context"], after["context"]
    out += [(key, b[key], a[key]) for key in CTX_KEYS if b[key] != a[key]]
    out += [(key, b[key], a[key]) for key in CTX_LAZY if arenas and b[key] != a[key]]
    return out


# ---- the subjects: each runs its calls twice in a row against one expectation ---------------------------------------------------
def _batches(items, size):
    return [items[k:k + size] for k in range(0, len(items), size)]


def encode_e1(ctx, pkg, oracle, batch):
    exp = hi.expectations(oracle)
    imgs = [i for _, i in hi.subject_images()]
    for b, w in zip(_batches(imgs, batch), _batches(exp["e1"], batch)):
        for again in range(2):
            assert ctx.encode_batch(b) == w, again


def encode_q(ctx, pkg, oracle, batch):
    exp = hi.expectations(oracle)
    imgs = [i for _, i in hi.subject_images()]
    try:
        for mode in ((0, 0), (1, 300)):                        # the host entropy stage, then the device rANS stage
            assert ctx.set_device_qcoder(*mode) == mode[0]
            for b, w in zip(_batches(imgs, batch), _batches(exp["q"], batch)):
                for again in range(2):
                    assert ctx.qencode_batch(b) == w, (mode, again)
    finally:
        ctx.set_device_qcoder(0)


def encode_modes(ctx, pkg, oracle, batch):
    exp = hi.expectations(oracle)
    imgs = [i for _, i in hi.subject_images()]
    for near, effort in hi.MODES:
        streams, recs = exp[(near, effort)]
        for b, ws, wr in zip(_batches(imgs, batch), _batches(streams, batch), _batches(recs, batch)):
            for again in range(2):
                got, rec = ctx.encode_modes(b, [near] * len(b), [effort] * len(b))
                assert got == ws, (near, effort, again)
                assert all(np.array_equal(r, w) for r, w in zip(rec, wr)), (near, effort, again)


def decode(ctx, pkg, oracle, batch):
    exp = hi.expectations(oracle)
    imgs = [i for _, i in hi.subject_images()]
    streams = exp["e1"] + exp["q"]
    want = [(i, 0, 1) for i in imgs] + [(i, 0, 0) for i in imgs]
    for near, effort in hi.MODES:
        streams = streams + exp[(near, effort)][0]
        want += [(r, near, effort) for r in exp[(near, effort)][1]]
    for k0 in range(0, len(streams), batch):                   # calls of `batch` streams: fewer job records than `decode` left
        for again in range(2):
            got = ctx.decode_batch(streams[k0:k0 + batch])
            for k, (g, (plane, near, effort)) in enumerate(zip(got, want[k0:k0 + batch]), k0):
                assert g is not None and np.array_equal(g[0], plane) and tuple(g[1:]) == (near, effort), (k, again)


def stage_arrays(ctx, pkg, oracle, batch):
    from test_gpu_parity import _assert_stage_parity
    for content, h, w in hi.STAGE_CASES:
        img = inputs.make(content, h, w)
        first = None
        for again in range(2):
            st = _assert_stage_parity(ctx, oracle, img, content)
            got = {name: ctx.debug_stage(img, name) for name in hi.STAGE_NAMES}
            t, ev = got["totals"], got["events"]
            assert t[1] == (st["y"] < ei.MAP_SYMS).sum() and t[2] == len(st["cu"]) == len(ev), (content, "totals: re-mapper records, bins")
            assert t[3] == ci.chain_layout(ev)[0].sum() and t[4] == 0, (content, "totals: touches, wide positions")
            # every context chain of these images is one block, which starts from the chain's own state: all "met", no table, no replay
            assert np.bincount(st["adr"].astype(np.int64)).max() <= 4096 and [int(v) for v in t[5:8]] == [len(np.unique(st["adr"])), 0, 0], (content, "totals: S2 blocks", t)
            if first is not None:
                assert all(np.array_equal(got[k], first[k]) for k in got), (content, "twice")
            first = got


def caller_records(ctx, pkg, oracle, batch):
    from test_chain_kernels import back, check_back, check_model, families, model_stages
    from test_entropy_front import check, front
    for model, name in hi.MODEL_FAMILIES:
        fam = families(model)[name]
        got = check_model(ctx, oracle, fam)
        again = model_stages(ctx, fam)
        assert got.keys() == again.keys() and all(np.array_equal(got[k], again[k]) for k in got), (model, name, "twice")
    for name in hi.BACK_FAMILIES:
        ev = back()[name]
        got = check_back(ctx, oracle, ev, name)
        again = ctx.debug_back_half(ev)
        assert all(np.array_equal(got[k], again[k]) for k in got), (name, "twice")
    fam = ei.sizes(6)[ei.SIZES.index(1025)]
    got = check(ctx, oracle, fam)
    again = front(ctx, fam)
    assert all(np.array_equal(got[k], again[k]) for k in got), (fam["name"], "twice")


def bands(ctx, pkg, oracle, batch):
    from test_band_front import encode
    img, want = hi.expectations(oracle)["band"]
    _, h, _, band_rows, every = hi.BAND_CASE
    for front in ("staged", "serial"):
        for again in range(2):
            s, _, rec, ix, _ = encode(ctx, img, band_rows, front, index_every=every)
            assert s == want and np.array_equal(rec, img), (front, again)
            assert ix is not None and ix == ctx.build_index(s, every), (front, again)
            assert np.array_equal(ctx.decode_indexed(s, ix), img), (front, again)
            for r0, r1 in ((0, 1), (5, 16), (every, h), (h - 1, h)):
                assert np.array_equal(ctx.decode_rows(s, ix, r0, r1), img[r0:r1]), (front, again, r0, r1)


def index_unpack(ctx, pkg, oracle, batch):
    import index_pack_inputs as ipi
    import test_index_unpack_kernels as tuk
    case = next(c for c in tuk.CASES if c[2] == "real")         # an index the library accepts, NBLIC -e1
    c = ipi.cases()[case]
    count = len(c["bodies"])
    for again in range(2):
        for base, (walk, first_out) in ((1, (count, 0)), (2, (count, count - 1))):
            (result,) = ctx.debug_index_unpack([(c["packed"], base, walk, first_out)])
            tuk.check_task(case, result, walk, first_out, (case, base, walk, first_out, again))


@functools.lru_cache(maxsize=None)
def _cost_tasks(pkg):
    """The 65 x 130 and 130 x 65 tasks of the three plans' input modules with the host walks' sums, made once."""
    import color_plan_inputs as cpi
    import deep_inputs as di
    import stack_inputs as si
    from test_deep_host import host_cost
    pick = lambda tasks: [t for t in tasks if (t["rows"], t["cols"]) in hi.COST_SHAPES]
    color, stack, deep = pick(cpi.cost_tasks(pkg)), pick(si.cost_tasks(pkg)), pick(di.cost_tasks())
    assert len(color) == len(stack) == 24 and len(deep) == 2 * len(di.LAYOUTS)
    host = lambda fn, t: fn(t["raws"], t["rows"], t["cols"], t["fmt"], t["pitches"], t["steps"], t["scale"], t["bias"])
    return (color, [host(pkg.color_cost_host, t) for t in color], stack, [host(pkg.stack_cost_host, t) for t in stack],
            deep, [host_cost(pkg, t) for t in deep])


def costs(ctx, pkg, oracle, batch):
    color, want_color, stack, want_stack, deep, want_deep = _cost_tasks(pkg)
    for again in range(2):
        got = ctx.debug_color_cost(color)
        assert all(np.array_equal(g, w) for g, w in zip(got, want_color)) and len(got) == len(want_color), ("color", again)
        got = ctx.debug_stack_cost(stack)
        assert all(np.array_equal(g, w) for g, w in zip(got, want_stack)) and len(got) == len(want_stack), ("stack", again)
        assert all(np.array_equal(g, pkg.stack_cost_numpy(t["slices"])) for g, t in zip(got, stack)), ("stack, numpy", again)
        got = ctx.debug_deep_cost(deep)
        assert all(np.array_equal(g, w) for g, w in zip(got, want_deep)) and len(got) == len(want_deep), ("deep", again)


@functools.lru_cache(maxsize=None)
def _collect_deliver(pkg):
    """One collection task of collect_inputs (float16, three rows of 33, step 3, residue 6) and one delivery task as the
    deliver tests make them (bfloat16, a window of 3 x 33 of a 149-wide plane), with the host walks' bytes."""
    from collect_inputs import as_values, grid
    from test_deliver_host import ELEM, NORMS, expected, plane_of
    g = next(t for t in grid(1) if (t["rows"], t["cols"], t["layout"], t["residue"]) == (3, 33, 1, 6))
    ctask = dict(raw=g["raw"][g["residue"]:], rows=3, cols=33, fmt=1, pitch=g["pitch"], step=g["step"], scale=g["scale"], bias=g["bias"], base_offset=g["residue"] + 32)
    cwant = pkg.collect_host(ctask["raw"], 1, g["scale"], g["bias"], pitch=g["pitch"], step=g["step"], rows=3, cols=33).reshape(-1)
    assert np.array_equal(cwant, pkg.collect_numpy(as_values(g["bits"], 1), 1, g["scale"], g["bias"]).reshape(-1))
    fmt, window = 2, (1, 4, 3, 36)
    scale, bias = NORMS[1]
    dtask = dict(plane=plane_of(149), window=window, fmt=fmt, scale=scale, bias=bias, pitch=34 * ELEM[fmt], offset=ELEM[fmt], base_offset=7,
                 out_bytes=ELEM[fmt] + 2 * 34 * ELEM[fmt] + 33 * ELEM[fmt] + 21)
    dwant = pkg.deliver_host(dtask["plane"], window, fmt, scale, bias, pitch=dtask["pitch"], offset=dtask["offset"], out_bytes=dtask["out_bytes"])
    assert np.array_equal(dwant, expected(dtask["plane"], window, fmt, scale, bias, dtask["pitch"], dtask["offset"], dtask["out_bytes"]))
    return ctask, cwant, dtask, dwant


def collect_deliver(ctx, pkg, oracle, batch):
    ctask, cwant, dtask, dwant = _collect_deliver(pkg)
    guard, n = pkg.COLLECT_GUARD, cwant.size
    for again in range(2):
        (got,) = ctx.debug_collect([ctask])
        assert np.array_equal(got[guard:guard + n], cwant), again
        assert (got[:guard] == pkg.COLLECT_PATTERN).all() and (got[guard + n:] == pkg.COLLECT_PATTERN).all(), again
        (got,) = ctx.debug_deliver([dtask])
        assert np.array_equal(got, dwant), again


def device_coder(ctx, pkg, oracle, batch):
    """Last: the pack threads it starts stay with the context."""
    assert ctx.set_device_coder(2, 0) == 2
    encode_e1(ctx, pkg, oracle, batch)


SUBJECTS = (encode_e1, encode_q, encode_modes, decode, stage_arrays, caller_records, bands, index_unpack, costs, collect_deliver, device_coder)


def run_subjects(ctx, pkg, oracle, before=None, batch=hi.BATCH, arenas=False):
    """Every subject; behind each, the workspaces are where ``before`` found them (None: there is nothing to compare with)."""
    for subject in SUBJECTS:
        subject(ctx, pkg, oracle, batch)
        if before is not None:
            assert moved(before, ctx.debug_workspaces(), arenas) == [], subject.__name__


# ---- the tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("predecessor", hi.PREDECESSORS)
def test_subjects_behind_every_predecessor(pkg, oracle, live, predecessor):
    """One group of eight slots: exactly one workspace per slot.  ``fresh`` and ``dead_context`` have nothing to compare the
    memory with: their workspaces come from the allocator while the subjects run (the second's still holding the dead
    context's bytes), and which coded-bin buffer of a young pool an image takes, and so whether it has to grow, is a race."""
    if predecessor == "dead_context":
        hi.run_dead_context(pkg, lambda: make_ctx(pkg))
    ctx = make_ctx(pkg)
    try:
        hi.run_predecessor(predecessor, pkg, ctx)
        before = ctx.debug_workspaces()
        assert len(before["slots"]) == 1 and len(before["slots"][0]) == 8
        if predecessor in ("fresh", "dead_context"):
            assert all(s["px_cap"] == 0 and s["rec1"] == 0 for s in before["slots"][0]) and before["context"]["cbufs_held"] == 0
            run_subjects(ctx, pkg, oracle)
        else:
            assert all(s["px_cap"] >= 256 * 384 and s["ev_cap"] > 0 and s["rec1"] and s["events"] for s in before["slots"][0])
            assert before["slots"][0][0]["px_cap"] >= 1024 * 1024 and before["context"]["cbufs_held"] >= 8
            run_subjects(ctx, pkg, oracle, before, arenas=predecessor == "decode")
    finally:
        ctx.close()


@pytest.mark.parametrize("predecessor", ["hostile_e1", "flat"])
def test_subjects_in_two_groups(pkg, oracle, live, predecessor):
    """Two groups of four slots; the predecessor four times, so that both groups own a grown workspace whichever of them a
    call takes.  Calls of four images: one launch, four coded-bin buffers, which the predecessor's first launch allocated."""
    ctx = make_ctx(pkg, n_groups=2)
    try:
        for _ in range(4):
            hi.run_predecessor(predecessor, pkg, ctx)
        before = ctx.debug_workspaces()
        assert [len(g) for g in before["slots"]] == [4, 4]
        assert all(s["px_cap"] >= 256 * 384 and s["ev_cap"] > 0 for g in before["slots"] for s in g) and before["context"]["cbufs_held"] >= 4
        run_subjects(ctx, pkg, oracle, before, batch=4)
    finally:
        ctx.close()


def test_every_slot_takes_every_image_behind_another_neighbour(pkg, oracle, live):
    """The eight-image batch rotated by 0, 1, 3 and 5 places behind ``hostile_e1``: slot k takes image (k + r) mod 8."""
    imgs, want = hi.rotation_batch(), hi.expectations(oracle)["rotation"]
    ctx = make_ctx(pkg)
    try:
        hi.run_predecessor("hostile_e1", pkg, ctx)
        before = ctx.debug_workspaces()
        for r in hi.ROTATIONS:
            for again in range(2):
                assert ctx.encode_batch(imgs[r:] + imgs[:r]) == want[r:] + want[:r], (r, again)
            assert moved(before, ctx.debug_workspaces()) == [], r
    finally:
        ctx.close()


def test_a_small_pack_in_the_rows_of_a_large_one(pkg, oracle, live):
    """One coder thread, so eight images are a pack (where the host has AVX-512; elsewhere they go on their own, and the
    streams are held to the same bytes): a pack of eight hostile planes, then, in the same pack buffer, one of eight planes
    of 1 to 300 pixels -- k_pack_rows writes zero where a lane has no bin, over rows the first pack filled."""
    simd = pkg.range_code_multi([np.array([1], np.uint16)])[1] == 1
    big = list(hi.hostile_planes())
    small, want_small = hi.small_pack(), hi.expectations(oracle)["small_pack"]
    ctx = make_ctx(pkg, n_coders=1, n_host_buffers=8)
    try:
        got = ctx.encode_batch(big)
        assert ctx.takes() == ({8: 1} if simd else {1: 8})
        assert got[:2] == [oracle.encode(p, 0, 1)[0] for p in big[:2]]           # (two of them: the first pack is the predecessor here)
        before = ctx.debug_workspaces()
        assert before["context"]["pbufs_held"] == (1 if simd else 0)
        for again in range(2):
            assert ctx.encode_batch(small) == want_small, again
            assert ctx.takes() == ({8: 1} if simd else {1: 8})
            assert moved(before, ctx.debug_workspaces()) == [], again
        # the same two packs through the layout hook, which takes the pool's buffer too: the rows themselves
        rows, coded = ctx.debug_pack_rows(big)
        assert np.array_equal(rows, pkg.pack_groups_host(coded))
        rows, coded = ctx.debug_pack_rows(small)
        assert np.array_equal(rows, pkg.pack_groups_host(coded))
        for img, rec in zip(small, coded):
            st = oracle.stages(img)
            assert np.array_equal(rec, st["prob"].astype(np.uint16) | (st["ev_bin"].astype(np.uint16) << 15))
    finally:
        ctx.close()
