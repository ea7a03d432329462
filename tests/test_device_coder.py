"""GPU suite (-m gpu): the device range coder (csrc/device_coder.hip, k_range_code_lanes) on its own, lane by lane.
Context.debug_device_code launches the kernel once on jobs made here -- images on their own (u16 records) and lanes of
packs (13-bit rows) -- and every lane is compared byte for byte with the host coder of the same records
(pkg.range_code, which test_abi.py holds to the oracle), one test with the oracle's own bytes.

Everything the kernel may read but must not use is random: the records behind a stream's last bin up to the end of its
512-byte window or of its 64-bin group, the lanes of a pack that belong to no job, the rows of a short lane below its
last group.  All of it lies inside what the entry uploads; nothing here reads or writes out of bounds."""
import os
import subprocess
import sys

import numpy as np
import pytest

import inputs
from coder_inputs import every_probability, records, runs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 4 is the walk's unroll, 52 the words of a round and the codes of a group's low fields, 64 the group, 256 the round
LENGTHS = (0, 1, 3, 4, 5, 51, 52, 53, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4097)


class Wave:
    """The jobs of one launch, the packs they point into, and per job what it is and the records it has to code."""

    def __init__(self, pkg, seed):
        self.pkg, self.rng = pkg, np.random.default_rng(seed)
        self.jobs, self.packs, self.recs, self.what, self._lanes = [], [], [], [], []

    def single(self, rec, cap=None):
        """An image on its own: its window is filled up with random records."""
        n = len(rec)
        padded = np.concatenate([rec, records(self.rng, max(-(-n // 256), 1) * 256 - n)]).astype(np.uint16)
        return self._job(padded, rec, cap, f"single n={n}")

    def pack(self, lanes):
        """A pack of len(lanes) streams (None: a lane without records).  Every stream is filled up to the end of its last
        group with random records before it is laid out; then the rows of every lane below its last group, and the lanes
        that have no stream, up to the eighth, are random words."""
        full = [np.zeros(0, np.uint16) if r is None else np.concatenate([r, records(self.rng, -len(r) % 64)]).astype(np.uint16) for r in lanes]
        groups = max(len(f) // 64 for f in full)
        rows = (self.pkg.pack_groups_host(full) if groups else np.zeros(0, np.uint64)).reshape(groups, 13, 8)
        for lane in range(8):
            own = len(full[lane]) // 64 if lane < len(full) else 0
            rows[own:, :, lane] = self.rng.integers(0, 1 << 64, (groups - own, 13), dtype=np.uint64)
        self.packs.append(rows.reshape(-1))
        self._lanes.append(list(lanes))
        return len(self.packs) - 1

    def lane(self, pack, lane, cap=None):
        rec = self._lanes[pack][lane]
        return self._job((pack, lane), rec, cap, f"lane {lane} of pack {pack} ({len(self._lanes[pack])} streams) n={len(rec)}")

    def whole_pack(self, lanes):
        p = self.pack(lanes)
        return [self.lane(p, l) for l in range(len(lanes))]

    def _job(self, src, rec, cap, what):
        self.jobs.append([src, len(rec), 2 * len(rec) + 16 if cap is None else cap])      # (a bin makes 1.5 bytes at the most: 12 bits)
        self.recs.append(rec)
        self.what.append(what)
        return len(self.jobs) - 1

    def want(self):
        return [self.pkg.range_code(r) for r in self.recs]

    def run(self, ctx):
        return ctx.debug_device_code([tuple(j) for j in self.jobs], self.packs)

    def check(self, ctx, want=None):
        got, want = self.run(ctx), self.want() if want is None else want
        bad = [f"job {k}: {self.what[k]}" for k in range(len(want)) if got[k] != want[k]]
        assert not bad, bad
        return got


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(device=0, n_slots=2, n_coders=1, n_groups=1)
    yield c
    c.close()


def test_lengths(pkg, ctx):
    """Every length once as an image on its own, and as pack lanes: packs of 2..8 streams, three of each size, the lengths
    rotating through their lanes, so that every (pack size, lane) pair codes three different lengths.  126 jobs, one launch."""
    w = Wave(pkg, 1)
    for n in LENGTHS:
        w.single(records(w.rng, n))
    seen, at = {}, 0
    for size in range(2, 9):
        for rep in range(3):
            ns = [LENGTHS[(at + l) % len(LENGTHS)] for l in range(size)]
            at += size
            w.whole_pack([records(w.rng, n) for n in ns])
            for l, n in enumerate(ns):
                seen.setdefault((size, l), set()).add(n)
    assert len(seen) == 35 and all(len(v) == 3 for v in seen.values())
    assert set().union(*seen.values()) == set(LENGTHS)
    w.check(ctx)


@pytest.mark.parametrize("last", ("packed", "empty"))
@pytest.mark.parametrize("n_jobs", (1, 63, 64, 65, 130))
def test_wave_shapes(pkg, ctx, n_jobs, last):
    """Full and partial waves, one block and three: the lanes beyond n_jobs copy the last job -- a lane of a pack with bins
    of its own, or an empty stream -- and must write nothing."""
    w = Wave(pkg, 10 * n_jobs + (last == "empty"))
    lengths = (300, 0, 65, 1, 513, 64, 52, 256)
    k = 0
    while len(w.jobs) < n_jobs - 1:
        if k % 3 == 2 and n_jobs - 1 - len(w.jobs) >= 3:
            w.whole_pack([records(w.rng, lengths[(k + l) % 8]) for l in range(3)])
        else:
            w.single(records(w.rng, lengths[k % 8]))
        k += 1
    if last == "packed":
        p = w.pack([records(w.rng, n) for n in (64, 300, 700)])
        w.lane(p, 2)
    else:
        w.single(records(w.rng, 0))
    assert len(w.jobs) == n_jobs
    w.check(ctx)


def test_mixed_wave(pkg, ctx):
    """Singles and the lanes of three packs interleaved in job order, the lanes out of lane order; of the third pack, eight
    streams, only lanes 1 and 5 are jobs."""
    w = Wave(pkg, 3)
    a = w.pack([records(w.rng, n) for n in (700, 64, 0, 1300, 257)])
    b = w.pack([records(w.rng, n) for n in (53, 2000)])
    c = w.pack([None, records(w.rng, 1500), None, None, None, records(w.rng, 63), None, None])
    order = [("s", 400), (a, 3), (b, 1), ("s", 0), (c, 5), (a, 0), ("s", 1025), (a, 4), (a, 1), (c, 1), ("s", 52), (b, 0), (a, 2), ("s", 3000)]
    for what, v in order:
        if what == "s":
            w.single(records(w.rng, v))
        else:
            w.lane(what, v)
    w.check(ctx)


@pytest.mark.parametrize("long_one", ("single", "packed"))
def test_ragged_wave(pkg, ctx, long_one):
    """One lane of 13 000 bins, 51 rounds, among lanes of 0, 1, 64 and 300: the short streams' last window is fetched again
    round after round, a finished pack lane's rows read as zeros, and the wave walks with one lane for 49 rounds."""
    w = Wave(pkg, 4 + (long_one == "packed"))
    short = (0, 1, 64, 300)
    for n in short:
        w.single(records(w.rng, n))
    if long_one == "single":
        w.single(records(w.rng, 13000))
        w.whole_pack([records(w.rng, n) for n in short])
    else:
        lanes = [records(w.rng, n) for n in (1, 300, 13000, 0, 64)]
        p = w.pack(lanes)
        for l in (4, 2, 0, 3, 1):
            w.lane(p, l)
    for n in short:
        w.single(records(w.rng, n))
    w.check(ctx)


def test_extreme_probabilities(pkg, ctx):
    """Runs of probabilities 1 and 4095 (the likely bin: no byte for hundreds of bins; the unlikely one: a byte and a half
    per bin), and streams that hold every probability 1..4095 with both bins; each as an image on its own and packed."""
    w = Wave(pkg, 6)
    streams = [np.full(5000, 1 | (1 << 15), np.uint16), np.full(4097, 4095, np.uint16), runs(1, 9000), runs(2, 4096), np.full(6000, 1, np.uint16),
               runs(3, 12000), np.full(3000, 4095 | (1 << 15), np.uint16), runs(4, 65), every_probability(w.rng), every_probability(w.rng)[:4097]]
    for s in streams:
        w.single(s)
    w.whole_pack(streams[:5])
    w.whole_pack(streams[5:])
    got = w.check(ctx)
    assert max(len(b) for b in got) > 3000                      # the runs do produce bytes


def _capacity_wave(pkg):
    w = Wave(pkg, 7)
    for n in (0, 1, 64, 300, 1025, 3000):
        w.single(records(w.rng, n))
    w.single(runs(5, 2000))
    w.whole_pack([records(w.rng, n) for n in (257, 0, 52, 2500, 64, 1, 900, 4097)])
    w.whole_pack([records(w.rng, 700), runs(6, 1500), records(w.rng, 5)])
    w.single(records(w.rng, 513))
    w.single(records(w.rng, 4))
    return w


def test_capacity_that_fits_exactly(pkg, ctx):
    w = _capacity_wave(pkg)
    want = w.want()
    assert len(want) == 20
    for j, b in zip(w.jobs, want):
        j[2] = len(b)
    w.check(ctx, want)


def test_capacity_one_byte_short(pkg, ctx):
    """One single and one packed lane a byte short: those two do not fit, every other lane has its bytes -- and no guard
    byte behind any output has changed (the wrapper raises if one has)."""
    w = _capacity_wave(pkg)
    want = w.want()
    for j, b in zip(w.jobs, want):
        j[2] = len(b)
    short = (4, 10)                                             # a single of 1025 bins; lane 3 of the first pack, 2500 bins
    assert w.what[4].startswith("single n=1025") and w.what[10].startswith("lane 3 of pack 0") and len(w.recs[10]) == 2500
    for k in short:
        w.jobs[k][2] -= 1
        want[k] = None
    w.check(ctx, want)


def test_capacity_of_an_empty_stream(pkg, ctx):
    """An empty stream is its four flush bytes: no room for them in 0..3 bytes, exactly room in 4; single and packed."""
    w = Wave(pkg, 8)
    p = w.pack([records(w.rng, 0), records(w.rng, 200)])
    want = []
    for cap in (0, 1, 2, 3, 4):
        w.single(records(w.rng, 0), cap)
        w.lane(p, 0, cap)
        want += [bytes(4) if cap == 4 else None] * 2
    w.lane(p, 1)
    want.append(pkg.range_code(w.recs[-1]))
    assert pkg.range_code(np.zeros(0, np.uint16)) == bytes(4)
    w.check(ctx, want)


def test_capacity_far_too_small(pkg, ctx):
    """The 13 000-bin lane with room for 16 and 5 bytes: the output is full within the first hundred bins, the walk goes
    on for fifty rounds and writes nothing more; its neighbours are coded as ever."""
    w = Wave(pkg, 9)
    long_s, long_p = records(w.rng, 13000), records(w.rng, 13000)
    w.single(records(w.rng, 300))
    w.single(long_s, 16)
    p = w.pack([records(w.rng, 64), long_p, records(w.rng, 1000)])
    w.lane(p, 0)
    w.lane(p, 1, 5)
    w.lane(p, 2)
    want = w.want()
    assert len(want[1]) > 2000 and len(want[3]) > 2000          # a hundred times the room and more
    want[1] = want[3] = None
    w.check(ctx, want)


def test_oracle_bodies(pkg, ctx, oracle):
    """The oracle's own probabilities and bins, and its own bytes: no host coder in between."""
    w = Wave(pkg, 11)
    coded, want = [], []
    for content, h, wd in (("const", 1, 1), ("checker", 17, 13), ("noise", 40, 37), ("syn1", 64, 64)):
        st = oracle.stages(inputs.make(content, h, wd))
        coded.append(st["prob"].astype(np.uint16) | (st["ev_bin"].astype(np.uint16) << 15))
        want.append(st["body"])
    for c in coded:
        w.single(c)
    w.whole_pack(coded)
    w.check(ctx, want + want)


def test_refusals(pkg, ctx, oracle):
    """Every argument the entry has to refuse, and the context still encodes afterwards."""
    rng = np.random.default_rng(12)
    ok = records(rng, 256)
    lane1 = records(rng, 64)
    rows = pkg.pack_groups_host([records(rng, 64), lane1])     # one group: 104 words
    assert rows.size == 104
    refused = [
        ([(None, 0, 16)], []),                                 # neither records nor a pack lane
        ([((0, 8), 10, 64)], [rows]),                          # a lane above 7
        ([((0, -1), 10, 64)], [rows]),
        ([((1, 0), 10, 64)], [rows]),                          # a pack that is not there
        ([((-1, 0), 10, 64)], [rows]),
        ([((0, 0), 10, 64)], []),
        ([((0, 1), 65, 200)], [rows]),                         # two groups of bins, one group of rows
        ([((0, 1), 10, 64)], [rows[:103]]),                    # rows that are no whole number of groups
        ([(ok, 257, 600)], []),                                # records that end before their last window does
        ([(ok[:255], 1, 20)], []),
        ([(ok[:0], 0, 20)], []),                               # an empty stream without its one window
        ([], []),                                              # no job at all
        ([(ok, 10, 64), ((0, 0), 10, 64), (ok[:100], 10, 64)], [rows]),       # one bad job among good ones
    ]
    for jobs, packs in refused:
        with pytest.raises(ValueError):
            ctx.debug_device_code(jobs, packs)
    import ctypes as C
    one = (C.c_long * 1)()
    assert pkg.load_library().nblic_amd_debug_device_code(None, 1, None, None, None, None, 0, None, None, None, None, None, one) == -1
    assert pkg.load_library().nblic_amd_debug_device_code(ctx.handle, 1, None, None, None, None, 0, None, None, None, None, None, None) == -1
    assert ctx.debug_device_code([(ok, 256, 600), ((0, 1), 64, 200)], [rows]) == [pkg.range_code(ok), pkg.range_code(lane1)]
    imgs = [inputs.make(c, h, wd) for c, h, wd in (("syn1", 40, 50), ("noise", 17, 13), ("const", 1, 1))]
    assert ctx.encode_batch(imgs) == [oracle.encode(i, 0, 1)[0] for i in imgs]


_CHILD = (
    "import importlib, sys, numpy as np\n"
    "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "from coder_inputs import records\n"
    "pkg = importlib.import_module('nblic-image-compression_amd')\n"
    "rng = np.random.default_rng(13)\n"
    "a, b, c = records(rng, 512), records(rng, 128), records(rng, 64)\n"
    "ctx = pkg.Context(0, n_slots=2, n_coders=1, n_groups=1)\n"
    "got = ctx.debug_device_code([(a, 512, 2000), ((0, 1), 64, 300), ((0, 0), 128, 8)], [pkg.pack_groups_host([b, c])])\n"
    "assert got == [pkg.range_code(a), pkg.range_code(c), None], got\n"
    "try:\n"
    "    ctx.debug_device_code([((0, 9), 64, 300)], [pkg.pack_groups_host([b, c])])\n"
    "    raise SystemExit('not refused')\n"
    "except ValueError:\n"
    "    pass\n"
    "ctx.close()\n"
    "print('live', sorted(pkg.live_resources().items()))\n"
    "print('child ok')\n"
)


def test_resources():
    """In a process that has had this one context only: after a launch, a refusal and close(), every count of
    nblic_amd_debug_live is zero."""
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
    assert "live [('device', 0), ('locked', 0), ('pinned', 0), ('streams_events', 0)]" in r.stdout, r.stdout
