"""Inputs of the workspace-history tests (tests/test_workspace_history_host.py on the CPU, tests/test_workspace_history.py on the
GPU): PREDECESSORS, sequences of ordinary API calls that leave the grow-only device workspaces of a context full of other
images' bytes, and SUBJECTS, small calls whose results must not depend on what they find there.

Every byte a predecessor leaves is one a real caller could leave: there is no artificial fill.  Every predecessor but
``fresh`` and ``dead_context`` BEGINS with the ``hostile_e1`` batch: the GPU test asserts that a subject ran in the
predecessor's memory (``Context.debug_workspaces()`` unchanged), the debug hooks run on slot 0 of a group, and the largest
caller-made subject has 47 thousand records -- so every slot must own a workspace larger than any subject before the
predecessor's own calls put their leftovers on top of it.  The planes of that batch are ordered so that the 1024 x 1024 one
lands in slot 0, and one call on caller-made records follows them (``hostile_records``: no image reaches every context).

Not here: a predecessor of FAILED and ABORTED work (a batch with an output buffer one byte short, band encoders closed after
two bands).  On its first GPU runs a band of the subject behind it once ended in a device fault whose cause has not been
found by reading; until it is, nothing of it runs on a GPU.

The expectations of the subjects come from the oracle and the host walks alone, once per process (``expectations``)."""
import functools

import numpy as np

import inputs

PREDECESSORS = ("fresh", "hostile_e1", "flat", "q", "serial", "decode", "plans", "dead_context")

# ---- subjects -------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (3, 5), (17, 13), (40, 37), (64, 64), (5, 300)]
CONTENTS = ("syn1", "noise", "const")
MODES = [(2, 1), (0, 2), (3, 3), (9, 1)]
STAGE_CASES = [("syn1", 17, 13), ("noise", 40, 37)]
STAGE_NAMES = ("rec1", "pxs", "z", "cnt", "events", "coded", "totals")
MODEL_FAMILIES = [(0, "edge_65"), (0, "lengths_const"), (0, "remapper"), (1, "edge_65"), (1, "keys_high")]
BACK_FAMILIES = ["size_65", "staging", "alignment"]
BAND_CASE = ("syn1", 23, 150, 3, 7)                            # content, h, w, band_rows, index_every
COST_SHAPES = ((65, 130), (130, 65))                           # 2 x 3 and 3 x 2 cost tiles
BATCH = 8                                                      # images per subject call: one launch of a group of eight slots
ROTATIONS = (0, 1, 3, 5)


@functools.lru_cache(maxsize=None)
def subject_images():
    """[(name, plane)]: every shape in every content, read-only."""
    out = []
    for h, w in SHAPES:
        for c in CONTENTS:
            img = inputs.make(c, h, w)
            img.setflags(write=False)
            out.append(("%s_%dx%d" % (c, h, w), img))
    return out


def subject_batches():
    """The subject images in calls of at most BATCH."""
    imgs = [i for _, i in subject_images()]
    return [imgs[k:k + BATCH] for k in range(0, len(imgs), BATCH)]


def rotation_batch():
    """The eight-image subject batch of the rotation test: every shape, every content, the largest three twice over."""
    named = dict(subject_images())
    keys = ["syn1_1x1", "noise_3x5", "const_17x13", "syn1_40x37", "noise_64x64", "const_5x300", "syn1_64x64", "noise_5x300"]
    return [named[k] for k in keys]


@functools.lru_cache(maxsize=None)
def small_pack():
    """Eight planes of 1 to 300 pixels for the second pack of the pack test: lanes that end at very different bins."""
    shapes = [(1, 1), (1, 2), (3, 5), (7, 9), (10, 13), (12, 17), (15, 19), (15, 20)]
    return [inputs.make(CONTENTS[k % 3], h, w) if k % 2 else inputs.syn1(h, w, 70 + k) for k, (h, w) in enumerate(shapes)]


_exp = {}


def expectations(oracle):
    """What every encode / decode subject must give, from the oracle alone; computed once per process."""
    if not _exp:
        imgs = [i for _, i in subject_images()]
        _exp["e1"] = [oracle.encode(i, 0, 1)[0] for i in imgs]
        _exp["q"] = [oracle.qencode(i) for i in imgs]
        for near, effort in MODES:
            res = [oracle.encode(i, near, effort) for i in imgs]
            _exp[(near, effort)] = ([r[0] for r in res], [r[1] for r in res])
            for s, rec in zip(*_exp[(near, effort)]):                       # the oracle's decoder agrees with its encoder
                d = oracle.decode(s)
                assert d is not None and np.array_equal(d[0], rec) and d[1:] == (near, effort)
        for img, s, q in zip(imgs, _exp["e1"], _exp["q"]):
            assert np.array_equal(oracle.decode(s)[0], img) and np.array_equal(oracle.qdecode(q), img)
        _exp["rotation"] = [oracle.encode(i, 0, 1)[0] for i in rotation_batch()]
        _exp["small_pack"] = [oracle.encode(i, 0, 1)[0] for i in small_pack()]
        _exp["band"] = (band_plane(), oracle.encode(band_plane(), 0, 1)[0])
    return _exp


@functools.lru_cache(maxsize=None)
def band_plane():
    c, h, w, _, _ = BAND_CASE
    band = inputs.make(c, h, w)
    band.setflags(write=False)
    return band


# ---- predecessors ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hostile_planes(h=256, w=384, count=8, seed=31):
    """``count`` planes of random 0 / 255 pixels: symbols up to 255, the most bins a pixel can have, every context busy."""
    rng = np.random.default_rng(seed)
    out = [(rng.integers(0, 2, (h, w), dtype=np.uint8) * np.uint8(255)) for _ in range(count)]
    for p in out:
        p.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def hostile_e1_planes():
    """The ``hostile_e1`` batch: the 1024 x 1024 noise plane first (slot 0 of the first launch), then the eight hostile ones."""
    big = inputs.noise(1024, 1024, 11)
    big.setflags(write=False)
    return (big,) + hostile_planes()


@functools.lru_cache(maxsize=None)
def flat_planes():
    return (inputs.make("const", 300, 300), np.zeros((130, 1000), np.uint8), inputs.make("checker", 300, 300))


@functools.lru_cache(maxsize=None)
def serial_cases():
    """[(plane, near, effort)] of the ``serial`` predecessor; the 52000 columns take the rows-in-memory path."""
    small = hostile_planes(64, 96, 3, 32)
    return ((small[0], 9, 1), (small[1], 2, 2), (small[2], 1, 3), (inputs.syn1(3, 52000, 4), 0, 2))


def plan_sources():
    """Hostile 130 x 65 sources of the ``plans`` predecessor: [2, 3, 130, 65] uint8 frames (also two stacks of depth 3) and
    [2, 130, 65] uint16 deep images with both bytes hostile."""
    rng = np.random.default_rng(33)
    frames = rng.integers(0, 2, (2, 3, 130, 65), dtype=np.uint8) * np.uint8(255)
    deep = rng.integers(0, 2, (2, 130, 65)).astype(np.uint16) * np.uint16(0xFFFF) ^ rng.integers(0, 2, (2, 130, 65)).astype(np.uint16) * np.uint16(0x00FF)
    return frames, deep


def predecessor_planes(name):
    """The planes a predecessor codes, for the CPU test's measurements (``dead_context``: what the dead context coded)."""
    hostile = list(hostile_e1_planes())
    serial = [c[0] for c in serial_cases()]
    frames, _ = plan_sources()
    return {"fresh": [],
            "hostile_e1": hostile,
            "flat": hostile + list(flat_planes()),
            "q": hostile + 2 * list(hostile_planes()),
            "serial": hostile + serial,
            "decode": hostile + serial,
            "plans": hostile + [p for f in frames for p in f],
            "dead_context": hostile + 2 * list(hostile_planes()) + serial}[name]


@functools.lru_cache(maxsize=None)
def hostile_records():
    """chain_inputs' ``keys_all`` of model 0 as (x, rec1, adr): one record with an extreme error in each of the 2048 contexts.
    No image reaches them all -- the address holds eight comparisons of the prediction with its own taps, and over a hundred
    planes of every kind tried reach 1022 of the 2048 -- so the ``hostile_e1`` batch is followed by one
    ``debug_model_stages`` call on these records, which leaves every context's bias away from its first value."""
    import chain_inputs as ci
    fam = ci.model_families(0)["keys_all"]
    return fam["x"], ci.rec1_of(fam), fam["adr"]


def _run_hostile_e1(ctx):
    streams = ctx.encode_batch(list(hostile_e1_planes()))
    x, rec1, _ = hostile_records()
    ctx.debug_model_stages(0, x, rec1)
    return streams


def _run_q(ctx):
    ctx.set_device_qcoder(0)
    ctx.qencode_batch(list(hostile_planes()))
    ctx.set_device_qcoder(1, 300)
    ctx.qencode_batch(list(hostile_planes()))
    ctx.set_device_qcoder(0)


def _run_serial(ctx):
    cases = serial_cases()
    return ctx.encode_modes([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])[0]


def _run_decode(pkg, ctx):
    streams = _run_hostile_e1(ctx) + _run_serial(ctx)
    good = streams[-3]                                          # the 64 x 96 plane at (2, 2)
    res = ctx.decode_batch(streams + [good[: len(good) * 6 // 10], good[:20] + bytes(len(good) - 20)])
    assert all(r is not None for r in res[:len(streams)]) and res[len(streams)] is None
    pkg.decompress_bands(streams[1], band_rows=64, ctx=ctx)


def _run_plans(pkg, ctx):
    import torch
    frames, deep = plan_sources()
    dev = torch.from_numpy(frames).cuda()
    dev16 = torch.from_numpy(deep).cuda()
    torch.cuda.synchronize()
    ctx.color_plan(dev)
    ctx.stack_plan(dev)
    ctx.deep_plan(dev16)
    streams = ctx.encode_batch_from(dev[0])
    out = torch.zeros((3, 130, 65), dtype=torch.uint8, device="cuda")
    assert ctx.decode_batch_into(streams, out) is not None
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), frames[0])


def run_predecessor(name, pkg, ctx):
    """The calls of predecessor ``name`` on ``ctx``.  (``dead_context`` is run by the test on a context of its own, which it
    closes before it creates the subject's: see ``run_dead_context``.)"""
    if name in ("fresh", "dead_context"):
        return
    if name == "decode":
        return _run_decode(pkg, ctx)
    _run_hostile_e1(ctx)
    if name == "flat":
        ctx.encode_batch(list(flat_planes()))
    elif name == "q":
        _run_q(ctx)
    elif name == "serial":
        _run_serial(ctx)
    elif name == "plans":
        _run_plans(pkg, ctx)
    elif name != "hostile_e1":
        raise ValueError(name)


def run_dead_context(pkg, make_ctx):
    """A context that runs ``hostile_e1``, ``q`` and ``serial`` and is closed: what it held goes back to the allocator."""
    ctx = make_ctx()
    try:
        _run_hostile_e1(ctx)
        _run_q(ctx)
        _run_serial(ctx)
    finally:
        ctx.close()
